"""Tensor-level wrappers over the C-ABI (ldt_amd/_lib.py).  PyTorch is used only for device
memory and the current HIP stream; every arithmetic op below runs in libldt_hip.so."""
import collections

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RELU_BF16,
                   EPI_RESID_F32, check, lib)

__all__ = ["cast_pad_bf16", "gemm_bf16", "layernorm_modulate", "attention_fwd", "sgemm", "sinusoid",
           "sampler_step", "pndm_transfer", "lincomb4", "philox_normal", "pad64", "stream_ptr"]


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def pad64(k):
    return (k + 63) // 64 * 64


def _need(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.LdtHipError("%s must be a device tensor (got %s): the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))


def _rowmajor(t, name):
    if t.stride(-1) != 1:
        raise ValueError("%s must be contiguous in its last dim" % name)


def cast_pad_bf16(src, cols_pad=None, out=None):
    """fp32 [rows, cols] -> bf16 [rows, cols_pad] zero padded."""
    _need(src, torch.float32, "src")
    src2 = src.reshape(-1, src.shape[-1])
    _rowmajor(src2, "src")
    rows, cols = src2.shape
    cols_pad = cols_pad or (cols + 3) // 4 * 4
    if out is None:
        out = torch.empty((rows, cols_pad), dtype=torch.bfloat16, device=src.device)
    check(lib().ldt_cast_pad_bf16(_p(src2), src2.stride(0), _p(out), out.stride(0), rows, cols, cols_pad, stream_ptr()),
          "ldt_cast_pad_bf16")
    return out


def gemm_bf16(x, w, bias=None, epilogue=EPI_BF16, out=None, resid=None, skip=None, gate=None,
              gate_sample_stride=0, rows_per_sample=0, step_ptr=None, gate_step_stride=0, n=None):
    """out[M,N] = epi(x[M,K] @ w[N,K]^T + bias).  x, w bf16 (K % 64 == 0)."""
    _need(x, torch.bfloat16, "x"); _need(w, torch.bfloat16, "w"); _need(bias, torch.float32, "bias")
    _rowmajor(x, "x"); _rowmajor(w, "w")
    M, K = x.shape
    N = n if n is not None else w.shape[0]
    if w.shape[1] != K:
        raise ValueError("gemm: K mismatch x%s w%s" % (tuple(x.shape), tuple(w.shape)))
    if out is None:
        odt = torch.float32 if epilogue in (EPI_F32, EPI_RESID_F32) else torch.bfloat16
        out = torch.empty((M, N), dtype=odt, device=x.device)
    if epilogue == EPI_RESID_F32 and resid is None:
        resid = out
    check(lib().ldt_gemm_bf16(epilogue, _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0),
                              _p(resid), resid.stride(0) if resid is not None else 0,
                              _p(skip), skip.stride(0) if skip is not None else 0,
                              _p(gate), gate_sample_stride, rows_per_sample, _p(step_ptr), gate_step_stride,
                              M, N, K, stream_ptr()), "ldt_gemm_bf16")
    return out


GemmRoute = collections.namedtuple("GemmRoute", "family bm bn tiles_per_wg")
GEMM_FAMILIES = ("none", "256-one-tile", "256-multi-tile", "mid", "v1")


def gemm_route(epilogue, M, N, K, ldo=None, fold=0, max_wgs=0):
    """Which kernel gemm_bf16 (fold = 0) or the LN-folded producer / consumer (fold = 256 or 32: the statistics granule; producer when
    epilogue is EPI_RESID_F32) runs for this shape: the launcher's own decision (ldt_gemm_route), no launch.  -> GemmRoute(family in
    GEMM_FAMILIES, bm, bn, tiles_per_wg)."""
    r = int(lib().ldt_gemm_route(int(epilogue), int(M), int(N), int(K), int(N if ldo is None else ldo), int(fold), int(max_wgs)))
    return GemmRoute(GEMM_FAMILIES[r >> 28], (r >> 10) & 1023, r & 1023, (r >> 20) & 255)


def gemm_resid_lnstats(x, w, bias, out, ln_scale, gate=None, gate_sample_stride=0, rows_per_sample=0, step_ptr=None,
                       gate_step_stride=0, ln_step_stride=0, granule=256):
    """LN-folding producer: out += gate * (x @ w^T + bias) in place (fp32), and returns
    (xs bf16 [M,N] = out * (1 + ln_scale), stats fp32 [N/granule, M, 2] = per-row (sum, sumsq) of out per `granule` columns:
    256 = the 256-tile kernel, 32 = the small-batch kernel)."""
    _need(x, torch.bfloat16, "x"); _need(w, torch.bfloat16, "w"); _need(bias, torch.float32, "bias")
    _need(out, torch.float32, "out"); _need(ln_scale, torch.float32, "ln_scale")
    _rowmajor(x, "x"); _rowmajor(w, "w"); _rowmajor(out, "out")
    M, K = x.shape
    N = w.shape[0]
    xs = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    stats = torch.empty((N // granule, M, 2), dtype=torch.float32, device=x.device)
    check(lib().ldt_gemm_resid_lnstats(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), _p(gate),
                                       gate_sample_stride, rows_per_sample, _p(ln_scale), _p(xs), xs.stride(0), _p(stats),
                                       _p(step_ptr), gate_step_stride, ln_step_stride, M, N, K, N // granule, stream_ptr()),
          "ldt_gemm_resid_lnstats")
    return xs, stats


def gemm_lnfold(xs, w, stats, fold_s, fold_c, epilogue=EPI_BF16, step_ptr=None, fold_step_stride=0):
    """LN-folding consumer: bf16 [M,N] = epi(rstd * (xs @ w^T) - rstd * mean * fold_s + fold_c), (mean, rstd) per row
    from `stats` [K/256, M, 2] (256-tile kernels) or [K/32, M, 2] (small-batch kernels), as its producer wrote them."""
    _need(xs, torch.bfloat16, "xs"); _need(w, torch.bfloat16, "w"); _need(stats, torch.float32, "stats")
    _need(fold_s, torch.float32, "fold_s"); _need(fold_c, torch.float32, "fold_c")
    _rowmajor(xs, "xs"); _rowmajor(w, "w")
    M, K = xs.shape
    N = w.shape[0]
    if tuple(stats.shape) not in ((K // 256, M, 2), (K // 32, M, 2)) or not stats.is_contiguous():
        raise ValueError("gemm_lnfold: stats must be contiguous [K/256, M, 2] or [K/32, M, 2]")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=xs.device)
    check(lib().ldt_gemm_lnfold(epilogue, _p(xs), xs.stride(0), _p(w), w.stride(0), _p(stats), _p(fold_s), _p(fold_c), _p(out),
                                out.stride(0), _p(step_ptr), fold_step_stride, M, N, K, stats.shape[0], stream_ptr()), "ldt_gemm_lnfold")
    return out


def fold_mean_ratio(stats, K):
    """max over rows of mean^2 / variance from producer row statistics stats [K/256, M, 2] (one host sync)."""
    _need(stats, torch.float32, "stats")
    if stats.dim() != 3 or stats.shape[2] != 2 or not stats.is_contiguous():
        raise ValueError("fold_mean_ratio: stats must be contiguous [parts, M, 2]")
    out = torch.zeros(1, dtype=torch.float32, device=stats.device)
    check(lib().ldt_fold_mean_ratio(_p(stats), stats.shape[0], stats.shape[1], int(K), _p(out), stream_ptr()), "ldt_fold_mean_ratio")
    return float(out.item())


def layernorm_modulate(x, w=None, b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0,
                       step_ptr=None, mod_step_stride=0, out=None):
    """x fp32 [M,C] -> bf16 [M,C]: LN(eps 1e-6)[*w+b] then *(1+scale)+shift (per-sample vectors)."""
    _need(x, torch.float32, "x")
    _rowmajor(x, "x")
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=torch.bfloat16, device=x.device)
    check(lib().ldt_layernorm_modulate(_p(x), x.stride(0), _p(out), out.stride(0), _p(w), _p(b), _p(shift), _p(scale),
                                       mod_sample_stride, rows_per_sample, _p(step_ptr), mod_step_stride, M, Cc,
                                       stream_ptr()), "ldt_layernorm_modulate")
    return out


def attention_fwd(q, k, v, B, H, Nq, Nk, head_dim, out=None):
    """q [B*Nq, >=H*Dh] , k/v [B*Nk, ...] bf16 row views (heads at column h*Dh) -> O [B,H,Nq,Dh] bf16."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        _need(t, torch.bfloat16, nm); _rowmajor(t, nm)
    if out is None:
        out = torch.empty((B, H, Nq, head_dim), dtype=torch.bfloat16, device=q.device)
    if k.stride(0) * Nk != v.stride(0) * Nk:
        raise ValueError("attention: K and V must share the batch stride")
    check(lib().ldt_attention_fwd(_p(q), q.stride(0), q.stride(0) * Nq, _p(k), k.stride(0), _p(v), v.stride(0),
                                  k.stride(0) * Nk, _p(out), B, H, Nq, Nk, head_dim, stream_ptr()), "ldt_attention_fwd")
    return out


def sgemm(a, w, bias=None, act_in=ACT_NONE, act_out=ACT_NONE, out=None, out_bf16=False):
    """fp32: out[M,N] = act_out(act_in(a[M,K]) @ w[N,K]^T + bias)."""
    _need(a, torch.float32, "a"); _need(w, torch.float32, "w"); _need(bias, torch.float32, "bias")
    _rowmajor(a, "a"); _rowmajor(w, "w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("sgemm: K mismatch a%s w%s" % (tuple(a.shape), tuple(w.shape)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    else:
        out_bf16 = out.dtype == torch.bfloat16
    check(lib().ldt_sgemm(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), int(out_bf16),
                          act_in, act_out, M, N, K, stream_ptr()), "ldt_sgemm")
    return out


SGEMM_ROUTES = ("none", "sgemm_nt", "sgemm_mfma<128,128>", "sgemm_mfma<32,128>", "linear_smalln<4>", "linear_smalln<8>",
                "linear_smallk<4>", "linear_smallk<8>")


def sgemm_route_shape(M, N, K, lda=None, ldb=None, ldc=None, misaligned=0):
    """Which of its seven kernel forms sgemm runs for this shape: the launcher's own decision (ldt_sgemm_route), no launch, no device, no
    allocation.  Leading dimensions default to the dense ones; misaligned: bit 0 a, 1 w, 2 out, 3 bias not 16-byte aligned.
    -> index into SGEMM_ROUTES (0: no kernel takes it)."""
    return int(lib().ldt_sgemm_route(int(M), int(N), int(K), int(K if lda is None else lda), int(K if ldb is None else ldb),
                                     int(N if ldc is None else ldc), int(misaligned)))


def sgemm_route(a, w, bias=None, out=None):
    """sgemm_route_shape of the call sgemm(a, w, bias, out=out): strides and alignment from the tensors themselves (a fresh output is
    dense and aligned; the route does not depend on the activations or the output type)."""
    M, K = a.shape
    N = w.shape[0]
    mis = sum(bit for bit, t in ((1, a), (2, w), (4, out), (8, bias)) if t is not None and t.data_ptr() % 16)
    return sgemm_route_shape(M, N, K, a.stride(0), w.stride(0), N if out is None else out.stride(0), mis)


def sinusoid(t, freq):
    _need(t, torch.float32, "t"); _need(freq, torch.float32, "freq")
    e = torch.empty((t.numel(), 2 * freq.numel()), dtype=torch.float32, device=t.device)
    check(lib().ldt_sinusoid(_p(t), _p(freq), _p(e), t.numel(), freq.numel(), stream_ptr()), "ldt_sinusoid")
    return e


def sampler_step(x, params, coef, step, mode=0, noise=None, noise_step_stride=0, x_out=None, x_mean_out=None,
                 step_ptr=None, elem_offset=0, seed=0, philox_mul=1, philox_add=0, traj=None):
    """traj: optional fp32 [n_steps, x.numel()]; x after the step is also stored in row `step` (the sample loop's parity curve)."""
    _need(x, torch.float32, "x"); _need(params, torch.float32, "params"); _need(coef, torch.float32, "coef")
    _need(noise, torch.float32, "noise"); _need(traj, torch.float32, "traj")
    if x_out is None:
        x_out = torch.empty_like(x)
    if traj is not None and (traj.dim() != 2 or traj.shape[1] != x.numel() or not traj.is_contiguous()):
        raise ValueError("sampler_step: traj must be a contiguous fp32 [n_steps, %d] tensor, got %s" % (x.numel(), tuple(traj.shape)))
    head = (_p(x), _p(params), _p(noise), noise_step_stride, _p(x_out), _p(x_mean_out))
    tail = (_p(coef), _p(step_ptr), int(step), mode, x.numel(), elem_offset, seed, philox_mul, philox_add, stream_ptr())
    if traj is None:                                            # the two entry points differ by the traj operand alone
        check(lib().ldt_sampler_step(*head, *tail), "ldt_sampler_step")
    else:
        check(lib().ldt_sampler_step_traj(*head, _p(traj), *tail), "ldt_sampler_step_traj")
    return x_out


def _same_f32(ts, names, what):
    """Every tensor fp32 on the device, contiguous, of one shape."""
    for t, nm in zip(ts, names):
        _need(t, torch.float32, nm)
        if t.shape != ts[0].shape or not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous and of shape %s, got %s" % (what, nm, tuple(ts[0].shape), tuple(t.shape)))


def pndm_transfer(x, et, d, p, q, out=None):
    """PNDM transfer (diffusion_continuous.py:263-274): out = x + d * (p * x - q * et) in fp32, every product and sum rounded on its own
    (the reference's operation order).  x, et fp32 of one shape; d, p, q python floats holding fp32 values."""
    if out is None:
        _need(x, torch.float32, "x")
        out = torch.empty_like(x)
    _same_f32((x, et, out), ("x", "et", "out"), "pndm_transfer")
    check(lib().ldt_pndm_transfer(_p(x), _p(et), float(d), float(p), float(q), _p(out), x.numel(), stream_ptr()), "ldt_pndm_transfer")
    return out


def lincomb4(a, c, scale, out=None):
    """out = scale * (((c0 a0 + c1 a1) + c2 a2) + c3 a3) in fp32, left to right, no contraction (PNDM's Runge-Kutta average and 4-step
    combination, diffusion_continuous.py:291,300).  a: four fp32 tensors of one shape, c: four floats."""
    if len(a) != 4 or len(c) != 4:
        raise ValueError("lincomb4: four tensors with one coefficient each, got %d / %d" % (len(a), len(c)))
    if out is None:
        _need(a[0], torch.float32, "a[0]")
        out = torch.empty_like(a[0])
    _same_f32(tuple(a) + (out,), ("a[0]", "a[1]", "a[2]", "a[3]", "out"), "lincomb4")
    check(lib().ldt_lincomb4(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), float(c[0]), float(c[1]), float(c[2]), float(c[3]), float(scale),
                             _p(out), out.numel(), stream_ptr()), "ldt_lincomb4")
    return out


def batch_norm_sum(x, n_valid, per_sample, norms_scratch, sum_out):
    """sum_out[0] = sum over the first n_valid samples of ||x[b]||_2 (LangevinCorrector's torch.norm(...).mean() numerator)."""
    check(lib().ldt_batch_norm_sum(_p(x), int(n_valid), int(per_sample), _p(norms_scratch), _p(sum_out), stream_ptr()), "ldt_batch_norm_sum")


def langevin_coef(sums, n_total, snr, std_t, coef_out):
    """coef_out[4] = {1, -step/std, sqrt(2 step), 0} from the batch sums {sum ||params_b||, sum ||z_b||} over n_total samples."""
    check(lib().ldt_langevin_coef(_p(sums), int(n_total), float(snr), float(std_t), _p(coef_out), stream_ptr()), "ldt_langevin_coef")


def vpsde_score(params, t, beta0, beta1, sigma2_0):
    """-params / sqrt(var(t)) per sample (Trainer.score_fn, Latent_SDE_Trainer.py:57-61): params fp32 [B, ...], t fp32 [B]."""
    _need(params, torch.float32, "params"); _need(t, torch.float32, "t")
    params, t = params.contiguous(), t.contiguous()
    out = torch.empty_like(params)
    B = params.shape[0]
    check(lib().ldt_vpsde_score(_p(params), _p(t), float(beta0), float(beta1), float(sigma2_0), _p(out), B, params.numel() // B,
                                stream_ptr()), "ldt_vpsde_score")
    return out


def sde_score(params, t, kind, c0, c1, c2):
    """-params / sqrt(var(t)) for the SDE family `kind` (0 vpsde, 1 sub_vpsde, 2 vesde / geometric_sde; constants as in
    include/ldt_hip.h): params fp32 [B, ...], t fp32 [B]."""
    _need(params, torch.float32, "params"); _need(t, torch.float32, "t")
    params, t = params.contiguous(), t.contiguous()
    out = torch.empty_like(params)
    B = params.shape[0]
    check(lib().ldt_sde_score(_p(params), _p(t), int(kind), float(c0), float(c1), float(c2), _p(out), B, params.numel() // B,
                              stream_ptr()), "ldt_sde_score")
    return out


def _ode_vec(t, dtype, name, n=None):
    _need(t, dtype, name)
    if t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError("%s must be a contiguous 1-d tensor%s, got %s" % (name, "" if n is None else " of %d elements" % n, tuple(t.shape)))


def ode_stage(y, ks, coefs, h, y_out=None, x_out=None):
    """y_out = y + h * (((a0 k0 + a1 k1) + a2 k2) + ...) in float64, left to right over the 1..6 (`ks`, `coefs`) terms, and
    x_out = float32(y_out), the Score's input (ldt_ode_stage).  y, ks[i], y_out float64 [n], x_out float32 [n].  -> (y_out, x_out)."""
    n = y.numel()
    if not 1 <= len(ks) <= 6 or len(ks) != len(coefs):
        raise ValueError("ode_stage: 1..6 terms with one coefficient each, got %d / %d" % (len(ks), len(coefs)))
    _ode_vec(y, torch.float64, "y")
    for i, k in enumerate(ks):
        _ode_vec(k, torch.float64, "ks[%d]" % i, n)
    if y_out is None:
        y_out = torch.empty_like(y)
    if x_out is None:
        x_out = torch.empty(n, dtype=torch.float32, device=y.device)
    _ode_vec(y_out, torch.float64, "y_out", n); _ode_vec(x_out, torch.float32, "x_out", n)
    kp = [_p(k) for k in ks] + [0] * (6 - len(ks))
    a = [float(c) for c in coefs] + [0.0] * (6 - len(ks))
    check(lib().ldt_ode_stage(_p(y), *kp, *a, len(ks), float(h), _p(y_out), _p(x_out), n, stream_ptr()), "ldt_ode_stage")
    return y_out, x_out


def ode_rhs(x, p, f, g2, sd, k_out=None, is_score=False):
    """k_out = float64(-(f x - (0.5 g2) score)), score = -p / sd (p = the Score's params) or p itself (is_score): the reversed-time
    right-hand side of the probability-flow ODE in fp32, in the operation order of Trainer.score_fn + sample_model_ode's fun()
    (ldt_ode_rhs).  x, p float32 of n elements each, f / g2 / sd python floats holding fp32 values.  -> k_out float64 [n]."""
    _need(x, torch.float32, "x"); _need(p, torch.float32, "p")
    x, p = x.contiguous(), p.contiguous()
    n = x.numel()
    if p.numel() != n:
        raise ValueError("ode_rhs: x has %d elements, p %d" % (n, p.numel()))
    if k_out is None:
        k_out = torch.empty(n, dtype=torch.float64, device=x.device)
    _ode_vec(k_out, torch.float64, "k_out", n)
    check(lib().ldt_ode_rhs(_p(x), _p(p), int(bool(is_score)), float(f), float(g2), float(sd), _p(k_out), n, stream_ptr()), "ldt_ode_rhs")
    return k_out


def ode_scaled_sumsq(vs, coefs, ya, yb, atol, rtol, scratch=None, out=None):
    """out[0] = sum_i ((sum_j c_j v_j[i]) / (atol + rtol max(|ya[i]|, |yb[i]|)))^2 over 1..7 float64 vectors, reduced in a fixed
    order (ldt_ode_scaled_sumsq): the square of scipy's norm(error / scale).  scratch: float64 [>= 1] per-workgroup partials
    (_lib.ODE_SUMSQ_SCRATCH always suffice).  -> out, a float64 device tensor of one element (not synchronised)."""
    if not 1 <= len(vs) <= 7 or len(vs) != len(coefs):
        raise ValueError("ode_scaled_sumsq: 1..7 vectors with one coefficient each, got %d / %d" % (len(vs), len(coefs)))
    _ode_vec(ya, torch.float64, "ya")
    n = ya.numel()
    _ode_vec(yb, torch.float64, "yb", n)
    for i, v in enumerate(vs):
        _ode_vec(v, torch.float64, "vs[%d]" % i, n)
    if scratch is None:
        scratch = torch.empty(_lib.ODE_SUMSQ_SCRATCH, dtype=torch.float64, device=ya.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=ya.device)
    _ode_vec(scratch, torch.float64, "scratch"); _ode_vec(out, torch.float64, "out", 1)
    vp = [_p(v) for v in vs] + [0] * (7 - len(vs))
    c = [float(x) for x in coefs] + [0.0] * (7 - len(vs))
    check(lib().ldt_ode_scaled_sumsq(*vp, *c, len(vs), _p(ya), _p(yb), float(atol), float(rtol), _p(scratch), scratch.numel(), _p(out), n,
                                     stream_ptr()), "ldt_ode_scaled_sumsq")
    return out


def add_f32(a, b, out=None):
    """a + b, fp32, same shape."""
    _need(a, torch.float32, "a"); _need(b, torch.float32, "b")
    if a.shape != b.shape:
        raise ValueError("add_f32: shapes differ %s %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.empty_like(a)
    check(lib().ldt_add_f32(_p(a), _p(b), _p(out), a.numel(), stream_ptr()), "ldt_add_f32")
    return out


def group_stats(x, B, T, groups, eps=1e-6):
    """(mean, rstd) per (sample, group) of token-major fp32 rows x [B*T, C]: nn.GroupNorm's statistics on the reference's channels-first
    (B, C, N) tensor (tools/utils.py:177-179) -> fp32 [B, groups, 2]."""
    _need(x, torch.float32, "x"); _rowmajor(x, "x")
    C = x.shape[1]
    out = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    check(lib().ldt_group_stats(_p(x), x.stride(0), B, T, C, groups, float(eps), _p(out), stream_ptr()), "ldt_group_stats")
    return out


def norm_apply(x, stats=None, rows_per_stat=1, w=None, b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=1, out=None):
    """bf16 [M, C] = ((x - mean) rstd w + b)(1 + scale) + shift with (mean, rstd) from `stats` [S, G, 2] (None: identity norm)."""
    _need(x, torch.float32, "x"); _rowmajor(x, "x")
    M, C = x.shape
    if out is None:
        out = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    G = 0 if stats is None else stats.shape[1]
    check(lib().ldt_norm_apply(_p(x), x.stride(0), _p(out), out.stride(0), M, C, _p(stats), G, rows_per_stat, _p(w), _p(b), _p(shift), _p(scale),
                               mod_sample_stride, rows_per_sample, stream_ptr()), "ldt_norm_apply")
    return out


def block_activation_(x, kind):
    """x (bf16 [M, C], row-major view) = act(x) in place; kind = _lib.block_act_id(name) (> 0)."""
    _need(x, torch.bfloat16, "x")
    _rowmajor(x, "x")
    check(lib().ldt_block_activation(_p(x), x.stride(0), x.shape[0], x.shape[1], int(kind), stream_ptr()), "ldt_block_activation")
    return x


def widen_bf16(w):
    """bf16 -> fp32 copy (exact)."""
    _need(w, torch.bfloat16, "w")
    w = w.contiguous()
    out = torch.empty(w.shape, dtype=torch.float32, device=w.device)
    check(lib().ldt_widen_bf16(_p(w), _p(out), w.numel(), stream_ptr()), "ldt_widen_bf16")
    return out


def philox_normal(shape, device, seed, step=0, elem_offset=0):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib().ldt_philox_normal(_p(out), out.numel(), elem_offset, step, seed, stream_ptr()), "ldt_philox_normal")
    return out


# ----------------------------------------------------------------------------- Compressor encoder front end
# Upstream pointnet2_ops (the library every FPS call of the reference goes through — Compressor/layers.py:106, completion
# valsample :182-183; not vendored, not importable here — SURVEY §8c) ignores points with |p|^2 <= 1e-3; the reference's
# vendored twin (model/functional/src/sampling/sampling.cu) does not.  Default: upstream's rule ON (what a real checkpoint was
# trained with: centred ShapeNet clouds do have points that close to the origin).  LDT_FPS_SKIP_NEAR_ORIGIN=0, this flag, or
# skip_near_origin=False give the twin's behaviour.
FPS_SKIP_NEAR_ORIGIN = bool(int(__import__("os").environ.get("LDT_FPS_SKIP_NEAR_ORIGIN", "1")))


def fps(xyz, m, skip_near_origin=None):
    """xyz fp32 [B,n,3] -> int32 [B,m] (farthest point sampling, start index 0)."""
    _need(xyz, torch.float32, "xyz")
    xyz = xyz.contiguous()
    B, n, _ = xyz.shape
    idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
    skip = FPS_SKIP_NEAR_ORIGIN if skip_near_origin is None else bool(skip_near_origin)
    check(lib().ldt_fps(_p(xyz), B, n, m, int(skip), _p(idx), stream_ptr()), "ldt_fps")
    return idx


def norm_points(xyz):
    """Compressor.norm_pts (Network.py:170-174): xyz fp32 [B,n,3] -> (xyz - mean) / std per cloud and coordinate."""
    _need(xyz, torch.float32, "xyz")
    xyz = xyz.contiguous()
    out = torch.empty_like(xyz)
    check(lib().ldt_norm_points(_p(xyz), xyz.shape[0], xyz.shape[1], _p(out), stream_ptr()), "ldt_norm_points")
    return out


def mixture_seed(eps, sig, mu, logits):
    """InitialSet mixture rows (Compressor/layers.py:38-41): eps fp32 [rows, n_mix, D] -> [rows, D]."""
    for t, nm in ((eps, "eps"), (sig, "sig"), (mu, "mu"), (logits, "logits")):
        _need(t, torch.float32, nm)
    rows, n_mix, D = eps.shape
    out = torch.empty((rows, D), dtype=torch.float32, device=eps.device)
    check(lib().ldt_mixture_seed(_p(eps.contiguous()), _p(sig.contiguous()), _p(mu.contiguous()), _p(logits.contiguous()), n_mix, D, rows,
                                 _p(out), stream_ptr()), "ldt_mixture_seed")
    return out


def knn(xyz, centers, k, return_dist=False):
    """-> int32 [B,S,k] unordered nearest-neighbour sets (+ the [B,S,n] distances)."""
    _need(xyz, torch.float32, "xyz"); _need(centers, torch.float32, "centers")
    xyz, centers = xyz.contiguous(), centers.contiguous()
    B, n, _ = xyz.shape
    S = centers.shape[1]
    idx = torch.empty((B, S, k), dtype=torch.int32, device=xyz.device)
    dist = torch.empty((B, S, n), dtype=torch.float32, device=xyz.device) if return_dist else None
    check(lib().ldt_knn(_p(xyz), _p(centers), B, n, S, k, _p(idx), _p(dist), stream_ptr()), "ldt_knn")
    return (idx, dist) if return_dist else idx


def group_normalize(feat, xyz, fps_idx, knn_idx, alpha, beta, normalize="anchor", return_stats=False):
    """LocalGrouper rows ('anchor' or 'center' normalisation): -> bf16 [B*S*k, pad64(2D+3)].  return_stats: -> (U, fp64 [2B]), the per-cloud
    sums of (g - origin) and of its square that the normalisation was computed from (the kernels keep them as 2^-20 fixed point)."""
    B, n, D = feat.shape
    S, k = knn_idx.shape[1], knn_idx.shape[2]
    ldu = pad64(2 * D + 3)
    U = torch.empty((B * S * k, ldu), dtype=torch.bfloat16, device=feat.device)
    stats = torch.empty((2 * B,), dtype=torch.float64, device=feat.device)
    mode = {"anchor": 0, "center": 1}[normalize]
    gmean = torch.empty((B, S, D + 3), dtype=torch.float32, device=feat.device) if mode else None
    check(lib().ldt_group_normalize(_p(feat), _p(xyz), _p(fps_idx), _p(knn_idx), _p(alpha), _p(beta), _p(stats), B, n, S, k, D,
                                    _p(U), ldu, mode, _p(gmean), stream_ptr()), "ldt_group_normalize")
    if return_stats:
        return U, stats.view(torch.int64).double() * 2.0 ** -20                 # csrc/common.h: fx_load
    return U


GROUPER_FRAGS = 132                                      # 1 KB MFMA fragments in the fused grouper's weight image


def grouper_mlp(feat, xyz, fps_idx, knn_idx, alpha, beta, wimg, b1, b2, b3, out=None):
    """Grouping ('anchor' normalisation) + PreExtraction + max over the k neighbours (k = 8, 16 or a multiple of 32) in one
    kernel: feat fp32 [B,n,128], xyz [B,n,3], fps_idx [B,S], knn_idx [B,S,k] -> fp32 [B*S, 128].  wimg: bf16 fragment image
    (include/ldt_hip.h: ldt_grouper_mlp) built by LocalGrouper.pack.  out: a contiguous fp32 [B*S, 128] tensor (or view) to write into."""
    B, n, D = feat.shape
    S, k = knn_idx.shape[1], knn_idx.shape[2]
    for t, nm in ((feat, "feat"), (xyz, "xyz"), (alpha, "alpha"), (beta, "beta"), (b1, "b1"), (b2, "b2"), (b3, "b3")):
        _need(t, torch.float32, nm)
    _need(wimg, torch.bfloat16, "wimg")
    if not (feat.is_contiguous() and xyz.is_contiguous() and fps_idx.is_contiguous() and knn_idx.is_contiguous() and wimg.is_contiguous()):
        raise ValueError("grouper_mlp: operands must be contiguous")
    if wimg.numel() != GROUPER_FRAGS * 512 or alpha.numel() != D + 3 or beta.numel() != D + 3 or min(b1.numel(), b2.numel(), b3.numel()) < D:
        raise ValueError("grouper_mlp: weight image / affine vectors have the wrong size")
    if out is None:
        out = torch.empty((B * S, D), dtype=torch.float32, device=feat.device)
    else:
        _need(out, torch.float32, "out")
        if tuple(out.shape) != (B * S, D) or not out.is_contiguous() or out.device != feat.device:
            raise ValueError("grouper_mlp: out must be a contiguous fp32 [%d, %d] tensor on the operands' device" % (B * S, D))
    stats = torch.empty((2 * B,), dtype=torch.float64, device=feat.device)
    check(lib().ldt_grouper_mlp(_p(feat), _p(xyz), _p(fps_idx), _p(knn_idx), _p(alpha), _p(beta), _p(stats), B, n, S, k, D,
                                _p(wimg), _p(b1), _p(b2), _p(b3), _p(out), stream_ptr()), "ldt_grouper_mlp")
    return out


def gather_rows(src, idx):
    """src fp32 [B,n,C], idx int32 [B,S] -> [B,S,C]."""
    B, n, Cc = src.shape
    S = idx.shape[1]
    out = torch.empty((B, S, Cc), dtype=torch.float32, device=src.device)
    check(lib().ldt_gather_rows(_p(src.contiguous()), _p(idx), B, n, S, Cc, _p(out), stream_ptr()), "ldt_gather_rows")
    return out


def maxpool(x, G, n):
    """x [G*n, C] (bf16 or fp32, row stride respected) -> fp32 [G, C] max over n."""
    Cc = x.shape[1]
    out = torch.empty((G, Cc), dtype=torch.float32, device=x.device)
    check(lib().ldt_maxpool(_p(x), int(x.dtype == torch.bfloat16), x.stride(0), G, n, Cc, _p(out), stream_ptr()), "ldt_maxpool")
    return out


def actnorm_(x, shift, log_scale, B):
    """in place on x fp32 [B*T, C] with per-token parameters [T*C]."""
    check(lib().ldt_actnorm(_p(x), _p(shift), _p(log_scale), B, x.numel() // B, stream_ptr()), "ldt_actnorm")
    return x


def actnorm_bwd(dz, z, log_scale, B, dx=None, dshift=None, dlog_scale=None, want_sums=True):
    """Backward of actnorm_: dz, z (the forward's OUTPUT) fp32 with B samples of dz.numel() // B elements, log_scale fp32 [per_sample] ->
    (dx, dshift, dlog_scale): dx = dz exp(-log_scale) (`dx` given: written there, dz itself allowed), dshift = -sum_b dx and
    dlog_scale = -sum_b dz z into the buffers given or fresh ones (want_sums False: dx only, both None)."""
    for t, nm in ((dz, "dz"), (z, "z"), (log_scale, "log_scale"), (dx, "dx"), (dshift, "dshift"), (dlog_scale, "dlog_scale")):
        _need(t, torch.float32, nm)
    if not dz.is_contiguous() or not z.is_contiguous() or dz.shape != z.shape:
        raise ValueError("actnorm_bwd: dz %s and z %s must be contiguous and of one shape" % (tuple(dz.shape), tuple(z.shape)))
    per = dz.numel() // max(int(B), 1)
    if B < 1 or per < 1 or per * B != dz.numel() or log_scale.numel() != per or not log_scale.is_contiguous():
        raise ValueError("actnorm_bwd: %d elements in B = %d samples with log_scale %s" % (dz.numel(), B, tuple(log_scale.shape)))
    if dx is None:
        dx = torch.empty_like(dz)
    elif not dx.is_contiguous() or dx.numel() != dz.numel():
        raise ValueError("actnorm_bwd: dx %s is not contiguous with dz's %d elements" % (tuple(dx.shape), dz.numel()))
    if want_sums:
        dshift = torch.empty(per, dtype=torch.float32, device=dz.device) if dshift is None else dshift
        dlog_scale = torch.empty(per, dtype=torch.float32, device=dz.device) if dlog_scale is None else dlog_scale
        for t in (dshift, dlog_scale):
            if not t.is_contiguous() or t.numel() != per:
                raise ValueError("actnorm_bwd: a sum buffer is %s, not contiguous with %d elements" % (tuple(t.shape), per))
    else:
        dshift = dlog_scale = None
    check(lib().ldt_actnorm_bwd(_p(dz), _p(z), _p(log_scale), B, per, _p(dx), _p(dshift), _p(dlog_scale), stream_ptr()), "ldt_actnorm_bwd")
    return dx, dshift, dlog_scale


# ---- training the Compressor's front: training-mode BatchNorm + ReLU, the max with its arg-max, the 'anchor' grouping's backward
def _rows2d(t, name, dtypes=(torch.float32,)):
    if t.dim() != 2:
        raise ValueError("%s must be [rows, columns], got %s" % (name, tuple(t.shape)))
    if not t.is_cuda:
        raise _lib.LdtHipError("%s must be a device tensor (got %s): the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    _rowmajor(t, name)


def _vecC(t, C, name):
    _need(t, torch.float32, name)
    if t is not None and (t.numel() != C or not t.is_contiguous()):
        raise ValueError("%s must be contiguous with %d elements, got %s" % (name, C, tuple(t.shape)))


def bn_stats(x, eps=1e-5, running_mean=None, running_var=None, momentum=0.1, out=None):
    """Training-mode BatchNorm statistics of x fp32 [M, C] (M >= 2) -> fp32 [2, C] = (mean, rstd = 1 / sqrt(biased var + eps)).  running_mean /
    running_var fp32 [C]: updated in place as nn.BatchNorm1d does ((1 - momentum) r + momentum (mean | unbiased var))."""
    _rows2d(x, "x")
    M, Cc = x.shape
    if M < 2:
        raise ValueError("bn_stats: training-mode BatchNorm needs more than one value per channel, got %d rows" % M)
    _vecC(running_mean, Cc, "running_mean"); _vecC(running_var, Cc, "running_var")
    if out is None:
        out = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    _need(out, torch.float32, "out")
    if tuple(out.shape) != (2, Cc) or not out.is_contiguous():
        raise ValueError("bn_stats: out must be a contiguous fp32 [2, %d]" % Cc)
    check(lib().ldt_bn_stats(_p(x), x.stride(0), M, Cc, float(eps), _p(out), _p(running_mean), _p(running_var), float(momentum), stream_ptr()),
          "ldt_bn_stats")
    return out


def _bn_operands(who, x, stats, gamma, beta):
    _rows2d(x, "x")
    M, Cc = x.shape
    _need(stats, torch.float32, "stats")
    if tuple(stats.shape) != (2, Cc) or not stats.is_contiguous():
        raise ValueError("%s: stats must be a contiguous fp32 [2, %d]" % (who, Cc))
    _vecC(gamma, Cc, "gamma"); _vecC(beta, Cc, "beta")
    return M, Cc


def bn_relu_fwd(x, stats, gamma, beta, out_bf16=True, cols_pad=None, out=None):
    """y = ReLU(gamma (x - mean) rstd + beta): x fp32 [M, C], stats from bn_stats -> bf16 (or fp32) [M, cols_pad], columns past C zero
    (cols_pad default: pad64(C) for bf16, C for fp32)."""
    M, Cc = _bn_operands("bn_relu_fwd", x, stats, gamma, beta)
    if out is None:
        cp = (pad64(Cc) if out_bf16 else Cc) if cols_pad is None else int(cols_pad)
        out = torch.empty((M, cp), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    else:
        _rows2d(out, "out", (torch.float32, torch.bfloat16))
        cp = out.shape[1] if cols_pad is None else int(cols_pad)
        if out.shape[0] != M or not Cc <= cp <= out.shape[1]:
            raise ValueError("bn_relu_fwd: out %s does not hold [%d, %d <= cols_pad = %d]" % (tuple(out.shape), M, Cc, cp))
    check(lib().ldt_bn_relu_fwd(_p(x), x.stride(0), M, Cc, _p(stats), _p(gamma), _p(beta), _p(out), out.stride(0), int(out.dtype == torch.bfloat16),
                                cp, stream_ptr()), "ldt_bn_relu_fwd")
    return out


def bn_relu_bwd(dy, x, stats, gamma, beta, dx=None, dgamma=None, dbeta=None):
    """Backward of bn_relu_fwd from dy fp32 [M, C] and the saved x -> (dx fp32 [M, C] (`dx` given: written there, dy itself allowed),
    dgamma, dbeta fp32 [C] into the buffers given or fresh ones)."""
    M, Cc = _bn_operands("bn_relu_bwd", x, stats, gamma, beta)
    _rows2d(dy, "dy")
    if tuple(dy.shape) != (M, Cc) or M < 2:
        raise ValueError("bn_relu_bwd: dy %s and x %s must share one [M >= 2, C] shape" % (tuple(dy.shape), tuple(x.shape)))
    if dx is None:
        dx = torch.empty((M, Cc), dtype=torch.float32, device=x.device)
    _rows2d(dx, "dx")
    if tuple(dx.shape) != (M, Cc):
        raise ValueError("bn_relu_bwd: dx %s is not [%d, %d]" % (tuple(dx.shape), M, Cc))
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device) if dgamma is None else dgamma
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device) if dbeta is None else dbeta
    _vecC(dgamma, Cc, "dgamma"); _vecC(dbeta, Cc, "dbeta")
    check(lib().ldt_bn_relu_bwd(_p(dy), dy.stride(0), _p(x), x.stride(0), M, Cc, _p(stats), _p(gamma), _p(beta), _p(dx), dx.stride(0), _p(dgamma),
                                _p(dbeta), stream_ptr()), "ldt_bn_relu_bwd")
    return dx, dgamma, dbeta


def maxpool_argmax(x, G, n, relu=False):
    """maxpool with the arg-max kept: x [G*n, C] (bf16 or fp32) -> (fp32 [G, C], int32 [G, C]); on equal values the smallest row index.
    relu: the values are ReLU(max) = max over the rows of ReLU(x); the arg-max is x's own."""
    _rows2d(x, "x", (torch.float32, torch.bfloat16))
    Cc = x.shape[1]
    if G < 1 or n < 1 or x.shape[0] != G * n:
        raise ValueError("maxpool_argmax: x %s is not [G = %d x n = %d, C]" % (tuple(x.shape), G, n))
    out = torch.empty((G, Cc), dtype=torch.float32, device=x.device)
    arg = torch.empty((G, Cc), dtype=torch.int32, device=x.device)
    check(lib().ldt_maxpool_argmax(_p(x), int(x.dtype == torch.bfloat16), x.stride(0), G, n, Cc, _p(out), _p(arg), int(bool(relu)), stream_ptr()),
          "ldt_maxpool_argmax")
    return out, arg


def maxpool_relu_bwd(d_out, out, arg, n, dz=None):
    """Backward of out = max over n rows of ReLU(z): d_out, out fp32 [G, C], arg int32 [G, C] -> dz fp32 [G*n, C], every element written."""
    _need(d_out, torch.float32, "d_out"); _need(out, torch.float32, "out"); _need(arg, torch.int32, "arg")
    G, Cc = out.shape
    for t, nm in ((d_out, "d_out"), (out, "out"), (arg, "arg")):
        if tuple(t.shape) != (G, Cc) or not t.is_contiguous():
            raise ValueError("maxpool_relu_bwd: %s %s is not a contiguous [%d, %d]" % (nm, tuple(t.shape), G, Cc))
    if dz is None:
        dz = torch.empty((G * n, Cc), dtype=torch.float32, device=out.device)
    _rows2d(dz, "dz")
    if n < 1 or tuple(dz.shape) != (G * n, Cc):
        raise ValueError("maxpool_relu_bwd: dz %s is not [%d, %d]" % (tuple(dz.shape), G * n, Cc))
    check(lib().ldt_maxpool_relu_bwd(_p(d_out), _p(out), _p(arg), G, n, Cc, _p(dz), dz.stride(0), stream_ptr()), "ldt_maxpool_relu_bwd")
    return dz


def knn_inverted_index(knn_idx, n):
    """The inverted index of knn_idx int32 [B, S, k] over the n points of each cloud -> (inv_start int32 [B, n + 1], inv_entry int32 [B, S k]):
    the entries s k + j with knn_idx[b, s, j] == p are inv_entry[b, inv_start[b, p]: inv_start[b, p + 1]], ascending.  Integer bookkeeping:
    a stable sort and a binary search in torch on the indices' device."""
    B = knn_idx.shape[0]
    flat = knn_idx.reshape(B, -1)
    vals, order = torch.sort(flat, dim=1, stable=True)
    edges = torch.arange(n + 1, dtype=flat.dtype, device=flat.device).unsqueeze(0).expand(B, -1).contiguous()
    start = torch.searchsorted(vals.contiguous(), edges)
    return start.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


def group_normalize_bwd(dU, feat, xyz, fps_idx, knn_idx, alpha, want_dfeat=True, index=None):
    """Backward of group_normalize('anchor'): dU fp32 | bf16 [B*S*k, >= 2D+3] -> (dalpha, dbeta fp32 [D+3], dfeat fp32 [B, n, D] or None).
    index: knn_inverted_index(knn_idx, n), built here when not given."""
    _rows2d(dU, "dU", (torch.float32, torch.bfloat16))
    for t, nm in ((feat, "feat"), (xyz, "xyz"), (alpha, "alpha")):
        _need(t, torch.float32, nm)
    _need(fps_idx, torch.int32, "fps_idx"); _need(knn_idx, torch.int32, "knn_idx")
    B, n, D = feat.shape
    S, k = knn_idx.shape[1], knn_idx.shape[2]
    if tuple(xyz.shape) != (B, n, 3) or tuple(fps_idx.shape) != (B, S) or knn_idx.shape[0] != B or alpha.numel() != D + 3:
        raise ValueError("group_normalize_bwd: feat %s, xyz %s, fps_idx %s, knn_idx %s, alpha %s do not fit" % (
            tuple(feat.shape), tuple(xyz.shape), tuple(fps_idx.shape), tuple(knn_idx.shape), tuple(alpha.shape)))
    if dU.shape[0] != B * S * k or dU.shape[1] < 2 * D + 3:
        raise ValueError("group_normalize_bwd: dU %s is not [%d, >= %d]" % (tuple(dU.shape), B * S * k, 2 * D + 3))
    if not (feat.is_contiguous() and xyz.is_contiguous() and fps_idx.is_contiguous() and knn_idx.is_contiguous() and alpha.is_contiguous()):
        raise ValueError("group_normalize_bwd: operands must be contiguous")
    dalpha = torch.empty(D + 3, dtype=torch.float32, device=feat.device)
    dbeta = torch.empty(D + 3, dtype=torch.float32, device=feat.device)
    dfeat = start = entry = None
    if want_dfeat:
        start, entry = knn_inverted_index(knn_idx, n) if index is None else index
        _need(start, torch.int32, "inv_start"); _need(entry, torch.int32, "inv_entry")
        if tuple(start.shape) != (B, n + 1) or tuple(entry.shape) != (B, S * k) or not (start.is_contiguous() and entry.is_contiguous()):
            raise ValueError("group_normalize_bwd: the inverted index is not ([%d, %d], [%d, %d])" % (B, n + 1, B, S * k))
        dfeat = torch.empty((B, n, D), dtype=torch.float32, device=feat.device)
    check(lib().ldt_group_normalize_bwd(_p(dU), int(dU.dtype == torch.bfloat16), dU.stride(0), _p(feat), _p(xyz), _p(fps_idx), _p(knn_idx), _p(start),
                                        _p(entry), _p(alpha), B, n, S, k, D, _p(dalpha), _p(dbeta), _p(dfeat), stream_ptr()), "ldt_group_normalize_bwd")
    return dalpha, dbeta, dfeat


def reparam(post, noise, out, lo, hi, want_stats=False):
    """post fp32 [rows, 2z], noise [rows, z] -> out[rows, z] (strided slice ok) = mu + exp(clamp(logvar)/2)*noise."""
    rows, z2 = post.shape
    z = z2 // 2
    mu = torch.empty((rows, z), dtype=torch.float32, device=post.device) if want_stats else None
    lv = torch.empty_like(mu) if want_stats else None
    check(lib().ldt_reparam(_p(post), _p(noise), _p(out), out.stride(0), _p(mu), _p(lv), rows, z, float(lo), float(hi),
                            stream_ptr()), "ldt_reparam")
    return mu, lv


# ----------------------------------------------------------------------------- held-out evaluation (eval_loss.hip)
def reparam_kl(post, noise, out, lo, hi, rows_per_sample, want_stats=False):
    """`reparam` plus the per-element log q(z) and KL of the draw (Network.py:12-19,221-224): post fp32 [rows, 2z], noise [rows, z] ->
    out[rows, z] (strided slice ok; bit-identical to `reparam`), returns (mu, logvar, kl [rows, z], logqz [rows, z], kl_sample_sum
    [rows / rows_per_sample]); mu / logvar None unless want_stats."""
    _need(post, torch.float32, "post"); _need(noise, torch.float32, "noise"); _need(out, torch.float32, "out")
    rows, z2 = post.shape
    z = z2 // 2
    if not (post.is_contiguous() and noise.is_contiguous() and noise.numel() == rows * z and out.shape == (rows, z) and out.stride(1) == 1):
        raise ValueError("reparam_kl: post [rows, 2z] and noise [rows, z] contiguous, out [rows, z] with unit column stride")
    dev = post.device
    mu = torch.empty((rows, z), dtype=torch.float32, device=dev) if want_stats else None
    lv = torch.empty_like(mu) if want_stats else None
    kl = torch.empty((rows, z), dtype=torch.float32, device=dev)
    lq = torch.empty_like(kl)
    ks = torch.empty((rows // max(int(rows_per_sample), 1),), dtype=torch.float32, device=dev)
    check(lib().ldt_reparam_kl(_p(post), _p(noise), _p(out), out.stride(0), _p(mu), _p(lv), _p(kl), _p(lq), _p(ks), rows,
                               int(rows_per_sample), z, float(lo), float(hi), stream_ptr()), "ldt_reparam_kl")
    return mu, lv, kl, lq, ks


def diffuse_q(x0, m, var, eta=None, *, seed=0, step=0):
    """x_t = x0 * m[b] + sqrt(var[b]) * eta (diffusion_continuous.py:78-81) with per-sample device scalars m, var [B]: x0 fp32
    [B, ...] -> (xt, eta).  eta None: drawn in the kernel from the Philox stream (seed, step) — the tensor
    `philox_normal(x0.shape, dev, seed, step)` would return — and handed back."""
    _need(x0, torch.float32, "x0"); _need(m, torch.float32, "m"); _need(var, torch.float32, "var"); _need(eta, torch.float32, "eta")
    x0 = x0.contiguous()
    B = x0.shape[0]
    m, var = m.reshape(-1).contiguous(), var.reshape(-1).contiguous()
    if m.numel() != B or var.numel() != B:
        raise ValueError("diffuse_q: m and var hold one scalar per sample (%d), got %d / %d" % (B, m.numel(), var.numel()))
    if eta is not None:
        if eta.shape != x0.shape:
            raise ValueError("diffuse_q: eta %s vs x0 %s" % (tuple(eta.shape), tuple(x0.shape)))
        eta = eta.contiguous()
    xt = torch.empty_like(x0)
    drawn = torch.empty_like(x0) if eta is None else None
    check(lib().ldt_diffuse_q(_p(x0), _p(eta), _p(m), _p(var), _p(xt), _p(drawn), B, x0.numel() // B, int(seed), int(step),
                              stream_ptr()), "ldt_diffuse_q")
    return xt, (drawn if eta is None else eta)


def dsm_loss(eta, params, weight=None, l1=False):
    """Denoising score-matching loss (Latent_SDE_Trainer.py:83-87): eta, params fp32 [B, ...], weight None or [B] ->
    (mean over everything, 0-dim; per-sample means [B]).  Both stay on the device."""
    _need(eta, torch.float32, "eta"); _need(params, torch.float32, "params"); _need(weight, torch.float32, "weight")
    if eta.shape != params.shape:
        raise ValueError("dsm_loss: eta %s vs params %s" % (tuple(eta.shape), tuple(params.shape)))
    eta, params = eta.contiguous(), params.contiguous()
    B = eta.shape[0]
    if weight is not None:
        weight = weight.reshape(-1).contiguous()
        if weight.numel() != B:
            raise ValueError("dsm_loss: weight holds one scalar per sample (%d), got %d" % (B, weight.numel()))
    per = torch.empty((B,), dtype=torch.float32, device=eta.device)
    mean = torch.empty((), dtype=torch.float32, device=eta.device)
    check(lib().ldt_dsm_loss(_p(eta), _p(params), _p(weight), B, eta.numel() // B, int(bool(l1)), _p(per), _p(mean), stream_ptr()),
          "ldt_dsm_loss")
    return mean, per


def nelbo_terms(eta, params, logqz, weight=None):
    """The sums of the latent NELBO's KL term (Hybrid_Trainer.py:139-143): eta, params, logqz fp32 [B, ...] of one shape, weight None or
    [B] -> (batch_sums [2] = (sum (eta - params)^2 * weight[b], sum logqz) over everything; sample_sums [B, 2], the same per sample).
    Both stay on the device."""
    _need(eta, torch.float32, "eta"); _need(params, torch.float32, "params"); _need(logqz, torch.float32, "logqz")
    _need(weight, torch.float32, "weight")
    if eta.shape != params.shape or eta.shape != logqz.shape:
        raise ValueError("nelbo_terms: eta %s vs params %s vs logqz %s" % (tuple(eta.shape), tuple(params.shape), tuple(logqz.shape)))
    eta, params, logqz = eta.contiguous(), params.contiguous(), logqz.contiguous()
    B = eta.shape[0]
    if weight is not None:
        weight = weight.reshape(-1).contiguous()
        if weight.numel() != B:
            raise ValueError("nelbo_terms: weight holds one scalar per sample (%d), got %d" % (B, weight.numel()))
    per = torch.empty((B, 2), dtype=torch.float32, device=eta.device)
    tot = torch.empty((2,), dtype=torch.float32, device=eta.device)
    check(lib().ldt_nelbo_terms(_p(eta), _p(params), _p(logqz), _p(weight), B, eta.numel() // max(B, 1), _p(per), _p(tot), stream_ptr()),
          "ldt_nelbo_terms")
    return tot, per


def occupancy_grid(pts, cells, counters=None, bernoulli=None):
    """evaluation_metrics.py:376-389 on the device: pts fp32 [S, n, 3], cells fp32 [G, 3] -> (counters, bernoulli), int32 [G] holding
    unsigned counts: points per nearest cell, and clouds with at least one point in the cell.  Given `counters` / `bernoulli` are added to."""
    _need(pts, torch.float32, "pts"); _need(cells, torch.float32, "cells")
    _need(counters, torch.int32, "counters"); _need(bernoulli, torch.int32, "bernoulli")
    if pts.dim() != 3 or pts.shape[-1] != 3 or cells.dim() != 2 or cells.shape[-1] != 3:
        raise ValueError("occupancy_grid: pts [S, n, 3] and cells [G, 3], got %s / %s" % (tuple(pts.shape), tuple(cells.shape)))
    pts, cells = pts.contiguous(), cells.contiguous()
    S, n, G = pts.shape[0], pts.shape[1], cells.shape[0]
    if counters is None:
        counters = torch.zeros((G,), dtype=torch.int32, device=pts.device)
    if bernoulli is None:
        bernoulli = torch.zeros((G,), dtype=torch.int32, device=pts.device)
    if counters.numel() != G or bernoulli.numel() != G or not (counters.is_contiguous() and bernoulli.is_contiguous()):
        raise ValueError("occupancy_grid: counters / bernoulli hold one contiguous count per cell (%d)" % G)
    check(lib().ldt_occupancy_grid(_p(pts), S, n, _p(cells), G, _p(counters), _p(bernoulli), stream_ptr()), "ldt_occupancy_grid")
    return counters, bernoulli


def chamfer(a, b):
    """a [B,na,3], b [B,nb,3] fp32 -> (dl [B,nb], dr [B,na]) squared nearest-neighbour distances."""
    a, b = a.contiguous(), b.contiguous()
    B, na, _ = a.shape
    nb = b.shape[1]
    dl = torch.empty((B, nb), dtype=torch.float32, device=a.device)
    dr = torch.empty((B, na), dtype=torch.float32, device=a.device)
    check(lib().ldt_chamfer(_p(a), _p(b), B, na, nb, _p(dl), _p(dr), stream_ptr()), "ldt_chamfer")
    return dl, dr


def chamfer_pairwise(x, y):
    """x [S,n,3], y [R,m,3] fp32 -> cd [S,R]: dl.mean(1) + dr.mean(1) of distChamfer for every cloud pair."""
    _need(x, torch.float32, "x"); _need(y, torch.float32, "y")
    x, y = x.contiguous(), y.contiguous()
    S, n, _ = x.shape
    R, m, _ = y.shape
    cd = torch.empty((S, R), dtype=torch.float32, device=x.device)
    check(lib().ldt_chamfer_pairwise(_p(x), _p(y), S, R, n, m, _p(cd), stream_ptr()), "ldt_chamfer_pairwise")
    return cd


def emd_approx(x, y, pairwise=False):
    """Approximate-matching transport cost (approxmatch + matchcost): x [S,n,3], y [R,m,3] fp32 ->
    [S] (pairs (x[b], y[b])) or [S,R] (pairwise)."""
    _need(x, torch.float32, "x"); _need(y, torch.float32, "y")
    x, y = x.contiguous(), y.contiguous()
    S, n, _ = x.shape
    R, m, _ = y.shape
    out = torch.empty((S, R) if pairwise else (S,), dtype=torch.float32, device=x.device)
    check(lib().ldt_emd_approx(_p(x), _p(y), S, R, n, m, int(pairwise), _p(out), stream_ptr()), "ldt_emd_approx")
    return out


def ln_mlp_resid_(x, w_up, b_up, w_dn, b_dn, ln_w=None, ln_b=None, shift=None, scale=None, gate=None,
                  mod_sample_stride=0, rows_per_sample=0, x_bf16_out=None, next_linear=None):
    """In place: x += gate * MLP(LN(x)[affine | modulated]) for C in {64, 128} channels (one fused kernel).
    x_bf16_out: optional bf16 [M, >=C] row-major tensor that receives a copy of the updated x in the same pass.
    next_linear: optional dict(w=bf16 [N, C], bias=fp32 [N] | None, ln_w=, ln_b= | shift=, scale=, mod_sample_stride=,
    rows_per_sample=, out= bf16 [M, N] row-major view to write into | None) — the following block's LayerNorm + first projection,
    computed on the updated rows by the same kernel; then returns (x, out bf16 [M, N]) instead of x."""
    _need(x, torch.float32, "x"); _rowmajor(x, "x")
    M, Cc = x.shape
    if x_bf16_out is not None:
        _need(x_bf16_out, torch.bfloat16, "x_bf16_out"); _rowmajor(x_bf16_out, "x_bf16_out")
        if x_bf16_out.shape[0] != M or x_bf16_out.shape[1] < Cc:
            raise ValueError("ln_mlp_resid_: x_bf16_out must be [M, >=C]")
    if tuple(w_up.shape) != (4 * Cc, Cc) or tuple(w_dn.shape) != (Cc, 4 * Cc) or not (w_up.is_contiguous() and w_dn.is_contiguous()):
        raise ValueError("ln_mlp_resid_: weights must be dense bf16 [4C][C] and [C][4C]")
    ldxb = 0 if x_bf16_out is None else x_bf16_out.stride(0)
    if next_linear is None:
        check(lib().ldt_ln_mlp_resid(_p(x), x.stride(0), M, Cc, _p(ln_w), _p(ln_b), _p(shift), _p(scale), _p(gate), mod_sample_stride,
                                     rows_per_sample, _p(w_up), _p(b_up), _p(w_dn), _p(b_dn), _p(x_bf16_out), ldxb, stream_ptr()),
              "ldt_ln_mlp_resid")
        return x
    nx = next_linear
    wn = nx["w"]
    _need(wn, torch.bfloat16, "next w")
    if wn.shape[1] != Cc or not wn.is_contiguous():
        raise ValueError("ln_mlp_resid_: next_linear w must be dense bf16 [N][C]")
    out = _bf16_rows_out(nx.get("out"), M, wn.shape[0], x.device, "ln_mlp_resid_: next_linear out")
    check(lib().ldt_ln_mlp_resid_next(_p(x), x.stride(0), M, Cc, _p(ln_w), _p(ln_b), _p(shift), _p(scale), _p(gate), mod_sample_stride,
                                      rows_per_sample, _p(w_up), _p(b_up), _p(w_dn), _p(b_dn), _p(x_bf16_out), ldxb,
                                      _p(nx.get("ln_w")), _p(nx.get("ln_b")), _p(nx.get("shift")), _p(nx.get("scale")),
                                      nx.get("mod_sample_stride", 0), nx.get("rows_per_sample", 0), _p(wn), _p(nx.get("bias")),
                                      wn.shape[0], _p(out), out.stride(0), stream_ptr()), "ldt_ln_mlp_resid_next")
    return x, out


def attention_oproj_resid_(q, k, v, B, H, Nq, Nk, head_dim, wo, bo, x, gate=None, gate_sample_stride=0):
    """In place: x[B*Nq, C] += gate * (Wo . Attn(q, k, v)' + bo) with the reference's raw head merge (quirk Q1), one kernel
    (Dh = 32, H in {2, 4}).  q [B*Nq, >=C], k/v [B*Nk, ...] bf16 row views; wo bf16 [C][C] dense."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (wo, "wo")):
        _need(t, torch.bfloat16, nm); _rowmajor(t, nm)
    _need(x, torch.float32, "x"); _rowmajor(x, "x")
    Cc = H * head_dim
    if tuple(wo.shape) != (Cc, Cc) or not wo.is_contiguous() or x.shape != (B * Nq, Cc):
        raise ValueError("attention_oproj_resid_: wo must be dense [C][C] and x [B*Nq, C]")
    check(lib().ldt_attention_oproj_resid(_p(q), q.stride(0), q.stride(0) * Nq, _p(k), k.stride(0), _p(v), v.stride(0),
                                          k.stride(0) * Nk, B, H, Nq, Nk, head_dim, _p(wo), _p(bo), _p(x), x.stride(0),
                                          _p(gate), gate_sample_stride, stream_ptr()), "ldt_attention_oproj_resid")
    return x


QKV_ATTENTION_ROUTES = ("two-kernels", "mid-self-32", "persistent-self-256", "mid-cross-32")


def qkv_attention_route(B, tokens, hidden, heads, K, cond_tokens=0, fold=0, max_wgs=0):
    """Which form qkv_attention (and the Score forward) runs for this shape: the launchers' own shape rules (ldt_qkv_attention_route), no
    launch.  fold: 0 plain, 32 / 256 = folded with statistics per that many columns.  -> index into QKV_ATTENTION_ROUTES."""
    return int(lib().ldt_qkv_attention_route(int(B), int(tokens), int(cond_tokens), int(hidden), int(heads), int(K), int(fold), int(max_wgs)))


def qkv_attention(x, w, B, tokens, heads, bias=None, stats=None, fold_s=None, fold_c=None, fold_step_stride=0, step_ptr=None,
                  kv_cond=None, cond_tokens=0, kv_batch_stride=None, max_wgs=0, out=None, qkv=None):
    """The q | k | v projection + attention step of a Score block as the forward launches it (ldt_qkv_attention): x [B*tokens, K] bf16 row
    view, w [3*hidden, K] (self-attention) or [hidden, K] with kv_cond [B*cond_tokens, >= 2*hidden] = the condition's K | V rows
    (cross-attention; kv_batch_stride: elements between samples when they are not cond_tokens rows apart); folded: x = the producer's xs, stats [K/256 or K/32, M, 2], fold_s / fold_c [(steps,) 3*hidden].
    qkv: the [M, 3*hidden] workspace the two-kernel path writes (a fused form leaves it alone).  -> O [B, heads, tokens, head_dim] bf16."""
    for t, nm in ((x, "x"), (w, "w"), (kv_cond, "kv_cond")):
        _need(t, torch.bfloat16, nm)
        if t is not None:
            _rowmajor(t, nm)
    for t, nm in ((bias, "bias"), (stats, "stats"), (fold_s, "fold_s"), (fold_c, "fold_c")):
        _need(t, torch.float32, nm)
    M, K = x.shape
    hidden = w.shape[0] if kv_cond is not None else w.shape[0] // 3
    if M != B * tokens or w.shape[1] != K or w.shape[0] != (hidden if kv_cond is not None else 3 * hidden) or hidden % heads:
        raise ValueError("qkv_attention: x%s w%s do not match B=%d tokens=%d heads=%d" % (tuple(x.shape), tuple(w.shape), B, tokens, heads))
    if kv_cond is not None:
        if kv_batch_stride is None:
            kv_batch_stride = kv_cond.stride(0) * cond_tokens
        if kv_cond.shape[1] < 2 * hidden or (B - 1) * kv_batch_stride + (cond_tokens - 1) * kv_cond.stride(0) + 2 * hidden > kv_cond.shape[0] * kv_cond.stride(0):
            raise ValueError("qkv_attention: kv_cond must hold B samples of cond_tokens rows [>= 2*hidden]")
    if stats is not None and (stats.dim() != 3 or tuple(stats.shape[1:]) != (M, 2) or not stats.is_contiguous()):
        raise ValueError("qkv_attention: stats must be contiguous [parts, M, 2]")
    if out is None:
        out = torch.empty((B, heads, tokens, hidden // heads), dtype=torch.bfloat16, device=x.device)
    if qkv is None:
        qkv = torch.empty((M, 3 * hidden), dtype=torch.bfloat16, device=x.device)
    _need(out, torch.bfloat16, "out"); _need(qkv, torch.bfloat16, "qkv")
    if not out.is_contiguous() or not qkv.is_contiguous() or qkv.numel() < M * 3 * hidden:
        raise ValueError("qkv_attention: out and qkv must be contiguous, qkv [M, 3*hidden]")
    check(lib().ldt_qkv_attention(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(stats), stats.shape[0] if stats is not None else 0,
                                  _p(fold_s), _p(fold_c), fold_step_stride, _p(kv_cond),
                                  kv_cond.stride(0) if kv_cond is not None else 0, kv_batch_stride or 0,
                                  _p(out), _p(qkv), B, tokens, cond_tokens, hidden, heads, K, max_wgs, _p(step_ptr), stream_ptr()),
          "ldt_qkv_attention")
    return out


def _bf16_rows_out(out, M, N, device, name):
    """A fresh bf16 [M, N], or the caller's: a row-major [M, N] view (row stride >= N) on `device`."""
    if out is None:
        return torch.empty((M, N), dtype=torch.bfloat16, device=device)
    _need(out, torch.bfloat16, name); _rowmajor(out, name)
    if tuple(out.shape) != (M, N) or out.device != device:
        raise ValueError("%s must be a bf16 [%d, %d] row-major tensor (or view) on the operands' device" % (name, M, N))
    return out


def ln_linear(x, w, bias=None, ln_w=None, ln_b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0, out=None):
    """bf16 [M,N] = LN(x)[affine | modulated] @ w[N,C]^T + bias for C in {64, 128} channels, N % 64 == 0 (one fused kernel).
    out: a bf16 [M, N] row-major tensor (or view, row stride >= N) to write into."""
    _need(x, torch.float32, "x"); _rowmajor(x, "x"); _need(w, torch.bfloat16, "w")
    M, Cc = x.shape
    N = w.shape[0]
    if w.shape[1] != Cc or not w.is_contiguous():
        raise ValueError("ln_linear: w must be dense bf16 [N][C]")
    out = _bf16_rows_out(out, M, N, x.device, "ln_linear: out")
    check(lib().ldt_ln_linear(_p(x), x.stride(0), M, Cc, _p(ln_w), _p(ln_b), _p(shift), _p(scale), mod_sample_stride, rows_per_sample,
                              _p(w), _p(bias), N, _p(out), out.stride(0), stream_ptr()), "ldt_ln_linear")
    return out


# ---- Score training: backward pieces and the optimizer (csrc/score_bwd.hip, attention_bwd.hip, optim.hip) -------------------------
def _f32_or_bf16(t, name):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))
    _need(t, t.dtype, name); _rowmajor(t, name)
    return int(t.dtype == torch.bfloat16)


def transpose_cast_bf16(src, rows_pad=None, out=None):
    """fp32 | bf16 [R, C] -> bf16 [C, rows_pad] = src^T, columns R.. zero (rows_pad defaults to pad64(R)): the operand form of W^T (dgrad)
    and of dY^T / X^T (wgrad, contraction over the R rows) for gemm_bf16."""
    is_bf16 = _f32_or_bf16(src, "src")
    if src.dim() != 2:
        raise ValueError("transpose_cast_bf16: src must be 2-D")
    R, Cc = src.shape
    rows_pad = pad64(R) if rows_pad is None else int(rows_pad)
    out = _bf16_rows_out(out, Cc, rows_pad, src.device, "transpose_cast_bf16: out")
    check(lib().ldt_transpose_cast_bf16(_p(src), is_bf16, src.stride(0), _p(out), out.stride(0), R, Cc, rows_pad, stream_ptr()),
          "ldt_transpose_cast_bf16")
    return out


def colsum(dy, out=None):
    """fp32 [C] = sum over the rows of dy fp32 | bf16 [M, C] (a bias gradient), fixed order."""
    is_bf16 = _f32_or_bf16(dy, "dy")
    M, Cc = dy.shape
    if out is None:
        out = torch.empty((Cc,), dtype=torch.float32, device=dy.device)
    _need(out, torch.float32, "out")
    check(lib().ldt_colsum(_p(dy), is_bf16, dy.stride(0), M, Cc, _p(out), stream_ptr()), "ldt_colsum")
    return out


def wgrad(dy, x, out=None):
    """dW fp32 [N, K] = dy[M, N]^T @ x[M, K] (operands fp32 | bf16, rounded to bf16) through the NT route: two transposing casts and
    gemm_bf16(EPI_F32) contracting over the M rows padded to a multiple of 64."""
    if dy.shape[0] != x.shape[0]:
        raise ValueError("wgrad: dy %s and x %s differ in rows" % (tuple(dy.shape), tuple(x.shape)))
    return gemm_bf16(transpose_cast_bf16(dy), transpose_cast_bf16(x), None, EPI_F32, out=out)


def dgrad(dy, w_t, epilogue=EPI_F32, out=None):
    """dX [M, K] = dy bf16 [M, N(pad 64)] @ W, with w_t = transpose_cast_bf16(W[N, K]) the bf16 [K, pad64(N)] panel."""
    return gemm_bf16(dy, w_t, None, epilogue, out=out)


def layernorm_modulate_bwd(x, dy, dx, scale=None, mod_sample_stride=0, rows_per_sample=None, want_mod=True, dshift=None, dscale=None):
    """Backward of layernorm_modulate (no affine): dx fp32 [M, C] += LayerNorm gradient; -> (dshift, dscale) fp32 [samples, C] summed
    over each sample's rows (None, None when not want_mod).  dshift / dscale: row views of one row stride to write into (column blocks
    of the modulation-row gradient)."""
    _need(x, torch.float32, "x"); _need(dy, torch.float32, "dy"); _need(dx, torch.float32, "dx"); _need(scale, torch.float32, "scale")
    for t, nm in ((x, "x"), (dy, "dy"), (dx, "dx")):
        _rowmajor(t, nm)
    M, Cc = x.shape
    if tuple(dy.shape) != (M, Cc) or tuple(dx.shape) != (M, Cc):
        raise ValueError("layernorm_modulate_bwd: x, dy, dx must share one [M, C] shape")
    rps = M if rows_per_sample is None else int(rows_per_sample)
    if rps <= 0 or M % rps:
        raise ValueError("layernorm_modulate_bwd: %d rows are not whole samples of %d" % (M, rps))
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    dsh = dsc = None
    if want_mod:
        dsh = torch.empty((M // rps, Cc), dtype=torch.float32, device=x.device) if dshift is None else dshift
        dsc = torch.empty((M // rps, Cc), dtype=torch.float32, device=x.device) if dscale is None else dscale
        for t, nm in ((dsh, "dshift"), (dsc, "dscale")):
            _need(t, torch.float32, nm); _rowmajor(t, nm)
            if tuple(t.shape) != (M // rps, Cc) or t.stride(0) != dsh.stride(0):
                raise ValueError("layernorm_modulate_bwd: %s must be [%d, %d] with the row stride of dshift" % (nm, M // rps, Cc))
    check(lib().ldt_layernorm_modulate_bwd(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(scale), mod_sample_stride, rps, _p(dx), dx.stride(0),
                                           _p(dsh), _p(dsc), dsh.stride(0) if want_mod else 0, _p(stats), M, Cc, stream_ptr()),
          "ldt_layernorm_modulate_bwd")
    return dsh, dsc


def gelu_bwd(u, dh, out=None):
    """bf16 [M, C] = dh * GELU'(u) on the saved bf16 pre-activation u; dh fp32 | bf16."""
    _need(u, torch.bfloat16, "u"); _rowmajor(u, "u")
    is_bf16 = _f32_or_bf16(dh, "dh")
    M, Cc = u.shape
    if tuple(dh.shape) != (M, Cc):
        raise ValueError("gelu_bwd: u %s vs dh %s" % (tuple(u.shape), tuple(dh.shape)))
    out = _bf16_rows_out(out, M, Cc, u.device, "gelu_bwd: out")
    check(lib().ldt_gelu_bwd(_p(u), u.stride(0), _p(dh), is_bf16, dh.stride(0), _p(out), out.stride(0), M, Cc, stream_ptr()), "ldt_gelu_bwd")
    return out


def gate_residual_bwd(dy, gate, a=None, gate_sample_stride=None, rows_per_sample=None, out=None, dgate=None):
    """y = x + gate[s] * a: -> (da bf16 [M, C] = dy * gate[s], dgate fp32 [samples, C] = per-sample sum of dy * a, or None without a).
    gate: fp32 [samples, >= C] rows (a view into the modulation rows is fine)."""
    _need(dy, torch.float32, "dy"); _rowmajor(dy, "dy"); _need(gate, torch.float32, "gate"); _rowmajor(gate, "gate")
    M, Cc = dy.shape
    rps = M if rows_per_sample is None else int(rows_per_sample)
    if rps <= 0 or M % rps:
        raise ValueError("gate_residual_bwd: %d rows are not whole samples of %d" % (M, rps))
    gate = gate.reshape(-1, gate.shape[-1])
    gss = (gate.stride(0) if gate.shape[0] > 1 else 0) if gate_sample_stride is None else int(gate_sample_stride)
    if gate.shape[0] not in (1, M // rps) or gate.shape[1] < Cc:
        raise ValueError("gate_residual_bwd: gate %s for %d samples of %d channels" % (tuple(gate.shape), M // rps, Cc))
    a_bf16 = 0
    if a is not None:
        a_bf16 = _f32_or_bf16(a, "a")
        if tuple(a.shape) != (M, Cc):
            raise ValueError("gate_residual_bwd: a %s vs dy %s" % (tuple(a.shape), tuple(dy.shape)))
        if dgate is None:
            dgate = torch.empty((M // rps, Cc), dtype=torch.float32, device=dy.device)
        _need(dgate, torch.float32, "dgate"); _rowmajor(dgate, "dgate")
        if tuple(dgate.shape) != (M // rps, Cc):
            raise ValueError("gate_residual_bwd: dgate must be [%d, %d]" % (M // rps, Cc))
    elif dgate is not None:
        raise ValueError("gate_residual_bwd: dgate needs the branch output a")
    out = _bf16_rows_out(out, M, Cc, dy.device, "gate_residual_bwd: out")
    check(lib().ldt_gate_residual_bwd(_p(dy), dy.stride(0), _p(a), a_bf16, a.stride(0) if a is not None else 0, _p(gate), gss, rps, _p(out),
                                      out.stride(0), _p(dgate), dgate.stride(0) if dgate is not None else 0, M, Cc, stream_ptr()),
          "ldt_gate_residual_bwd")
    return out, dgate


def silu_bwd(c, dy, want_act=False):
    """fp32 dc = dy * SiLU'(c); with want_act -> (dc, SiLU(c)) — the operand of the next Linear's weight gradient."""
    _need(c, torch.float32, "c"); _need(dy, torch.float32, "dy")
    if c.shape != dy.shape:
        raise ValueError("silu_bwd: c %s vs dy %s" % (tuple(c.shape), tuple(dy.shape)))
    c, dy = c.contiguous(), dy.contiguous()
    out = torch.empty_like(c)
    act = torch.empty_like(c) if want_act else None
    check(lib().ldt_silu_bwd(_p(c), _p(dy), _p(out), _p(act), c.numel(), stream_ptr()), "ldt_silu_bwd")
    return (out, act) if want_act else out


def dsm_loss_bwd(eta, params, weight=None, l1=False):
    """Gradient of dsm_loss's mean with respect to params: fp32, the shape of params."""
    _need(eta, torch.float32, "eta"); _need(params, torch.float32, "params"); _need(weight, torch.float32, "weight")
    if eta.shape != params.shape:
        raise ValueError("dsm_loss_bwd: eta %s vs params %s" % (tuple(eta.shape), tuple(params.shape)))
    eta, params = eta.contiguous(), params.contiguous()
    B = eta.shape[0]
    if weight is not None:
        weight = weight.reshape(-1).contiguous()
        if weight.numel() != B:
            raise ValueError("dsm_loss_bwd: weight holds one scalar per sample (%d), got %d" % (B, weight.numel()))
    out = torch.empty_like(params)
    check(lib().ldt_dsm_loss_bwd(_p(eta), _p(params), _p(weight), B, eta.numel() // B, int(bool(l1)), _p(out), stream_ptr()), "ldt_dsm_loss_bwd")
    return out


def embedding_grad(dc, label, n_classes):
    """fp32 [n_classes, D]: row k = the sum of dc[b] over the samples with label[b] == k, in the order of b."""
    _need(dc, torch.float32, "dc"); _rowmajor(dc, "dc")
    if not label.is_cuda:
        raise _lib.LdtHipError("label must be a device tensor (got %s): the HIP path has no CPU fallback" % (label.device,))
    B, D = dc.shape
    label = label.reshape(-1).to(torch.int32).contiguous()
    if label.numel() != B:
        raise ValueError("embedding_grad: %d labels for %d rows" % (label.numel(), B))
    out = torch.empty((int(n_classes), D), dtype=torch.float32, device=dc.device)
    check(lib().ldt_embedding_grad(_p(dc), dc.stride(0), _p(label), B, D, int(n_classes), _p(out), stream_ptr()), "ldt_embedding_grad")
    return out


def _attention_bwd(fn, entry, q, k, v, o, do, B, H, lengths, head_dim, outs, extra=None, stats_out=None):
    """attention_bwd (lengths = (N,)) and attention_bwd_cross ((Nq, Nk)): the operand checks, outs(H*head_dim) -> (dq, dk, dv) bf16 row
    views, the statistics buffer and the call of `entry`, which takes the lengths as given.  extra(Cc) -> arguments between head_dim and
    the stream (attention_bwd_long's scratch).  stats_out: a contiguous fp32 [B, H, Nq, 2] tensor that receives the row statistics (L, D)
    in place of a buffer of this call's own."""
    Nq, Nk, cross = lengths[0], lengths[-1], len(lengths) == 2
    if head_dim not in (8, 16, 32, 64):
        raise ValueError("%s: head_dim %r is not 8, 16, 32 or 64" % (fn, head_dim))
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (o, "o"), (do, "do")):
        _need(t, torch.bfloat16, nm); _rowmajor(t, nm)
    if not (o.is_contiguous() and do.is_contiguous()) or o.numel() != B * H * Nq * head_dim or do.numel() != o.numel():
        raise ValueError("%s: o and do must be contiguous [B, H, %s, %d]" % (fn, "Nq" if cross else "N", head_dim))
    if k.stride(0) != v.stride(0):
        raise ValueError("%s: K and V must share the row stride" % fn)
    Cc = H * head_dim
    if cross and (q.shape[0] != B * Nq or k.shape[0] != B * Nk or v.shape[0] != B * Nk or min(q.shape[1], k.shape[1], v.shape[1]) < Cc):
        raise ValueError("%s: q %s, k %s, v %s for B %d, Nq %d, Nk %d, %d channels"
                         % (fn, tuple(q.shape), tuple(k.shape), tuple(v.shape), B, Nq, Nk, Cc))
    dq, dk, dv = outs(Cc)
    stats = torch.empty((B, H, Nq, 2), dtype=torch.float32, device=q.device) if stats_out is None else stats_out
    _need(stats, torch.float32, "stats_out")
    if not stats.is_contiguous() or stats.numel() != B * H * Nq * 2 or stats.device != q.device:
        raise ValueError("%s: stats_out must be a contiguous fp32 [B, H, Nq, 2] tensor on the operands' device" % fn)
    ldq, ldkv = dq.stride(0), dk.stride(0)
    check(getattr(lib(), entry)(_p(q), q.stride(0), q.stride(0) * Nq, _p(k), k.stride(0), _p(v), v.stride(0), k.stride(0) * Nk, _p(o), _p(do),
                                _p(stats), _p(dq), ldq, ldq * Nq, _p(dk), ldkv, _p(dv), ldkv, ldkv * Nk, B, H, *lengths, head_dim, *(extra(Cc) if extra else ()), stream_ptr()), entry)
    return dq, dk, dv


def attention_bwd(q, k, v, o, do, B, H, N, head_dim=64, out=None):
    """Self-attention backward: q, k, v bf16 row views [B*N, >= H*head_dim] as attention_fwd takes them, o and do the contiguous bf16
    [B, H, N, head_dim] buffers (quirk Q1: the raw (B*N, C) view).  -> (dq, dk, dv) bf16 views [B*N, H*head_dim] of one
    [B*N, 3*H*head_dim] tensor (`out` when given), the dY operand of the QKV projection's backward GEMMs.
    head_dim 64: ldt_attention_bwd; 8, 16 or 32: ldt_attention_bwd_narrow; anything else is a ValueError."""
    return _attention_bwd("attention_bwd", "ldt_attention_bwd" if head_dim == 64 else "ldt_attention_bwd_narrow", q, k, v, o, do, B, H, (N,),
                          head_dim, lambda Cc: _bf16_rows_out(out, B * N, 3 * Cc, q.device, "attention_bwd: out").split(Cc, 1))


def attention_bwd_cross(q, k, v, o, do, B, H, Nq, Nk, head_dim, dq_out=None, dkv_out=None):
    """Cross-attention backward (ldt_attention_bwd_cross): q bf16 row view [B*Nq, >= H*head_dim], k and v bf16 row views [B*Nk, ...] of one
    row stride, o and do the contiguous bf16 [B, H, Nq, head_dim] buffers (quirk Q1).  -> (dq, dk, dv): dq bf16 [B*Nq, H*head_dim] (`dq_out`
    when given), dk | dv the two halves of one bf16 [B*Nk, 2*H*head_dim] tensor (`dkv_out` when given), the dY operand of fc_kv's backward
    GEMMs.  head_dim 8, 16, 32 or 64; Nq != Nk allowed."""
    return _attention_bwd("attention_bwd_cross", "ldt_attention_bwd_cross", q, k, v, o, do, B, H, (Nq, Nk), head_dim,
                          lambda Cc: (_bf16_rows_out(dq_out, B * Nq, Cc, q.device, "attention_bwd_cross: dq_out"),)
                          + _bf16_rows_out(dkv_out, B * Nk, 2 * Cc, q.device, "attention_bwd_cross: dkv_out").split(Cc, 1))


def attention_bwd_long_scratch(B, H, Nq, Nk, head_dim=32):
    """floats of fp32 scratch attention_bwd_long needs: one [B, Nk, 2 * H * head_dim] partial of dK | dV per chunk of queries."""
    return -(-Nq // _lib.ATTN_BWD_LONG_CHUNK) * B * Nk * 2 * H * head_dim


def attention_bwd_long(q, k, v, o, do, B, H, Nq, Nk, dq_out=None, dkv_out=None, head_dim=32, scratch=None, stats_out=None):
    """attention_bwd_cross's contract on a long query axis (ldt_attention_bwd_long): head_dim 32 only, Nq <= ATTN_BWD_LONG_MAX_QUERIES,
    Nk <= ATTN_BWD_LONG_MAX_KEYS.  dK / dV are summed per chunk of ATTN_BWD_LONG_CHUNK queries into `scratch` (fp32, allocated here when
    not given: attention_bwd_long_scratch floats, laid out [chunk, B, Nk, 2 * H * 32] = dK unscaled | dV) and then added in chunk order.
    stats_out: a contiguous fp32 [B, H, Nq, 2] tensor that receives the row statistics (max + ln sum, rowsum(dO o O)) of every query."""
    need = attention_bwd_long_scratch(B, H, Nq, Nk, head_dim)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.float32, device=q.device)
    _need(scratch, torch.float32, "scratch")
    if not scratch.is_contiguous():
        raise ValueError("attention_bwd_long: scratch must be contiguous")
    return _attention_bwd("attention_bwd_long", "ldt_attention_bwd_long", q, k, v, o, do, B, H, (Nq, Nk), head_dim,
                          lambda Cc: (_bf16_rows_out(dq_out, B * Nq, Cc, q.device, "attention_bwd_long: dq_out"),)
                          + _bf16_rows_out(dkv_out, B * Nk, 2 * Cc, q.device, "attention_bwd_long: dkv_out").split(Cc, 1),
                          extra=lambda Cc: (_p(scratch), scratch.numel()), stats_out=stats_out)


def attention_bwd_wide_scratch(B, H, Nq, Nk, head_dim=32):
    """floats of fp32 scratch attention_bwd_wide needs: per chunk of keys, each query row's (maximum, sum) [B, H, Nq, 2] and one
    [B, Nq, H * head_dim] partial of dQ."""
    return -(-Nk // _lib.ATTN_BWD_WIDE_CHUNK) * B * H * Nq * (2 + head_dim)


def attention_bwd_wide(q, k, v, o, do, B, H, Nq, Nk, dq_out=None, dkv_out=None, head_dim=32, scratch=None, stats_out=None):
    """attention_bwd_cross's contract on a long KEY axis (ldt_attention_bwd_wide): head_dim 32 only, Nq <= ATTN_BWD_WIDE_MAX_QUERIES,
    Nk <= ATTN_BWD_WIDE_MAX_KEYS.  The row statistics and dQ are formed per chunk of ATTN_BWD_WIDE_CHUNK keys in `scratch` (fp32, allocated
    here when not given: attention_bwd_wide_scratch floats, laid out [chunk, B, H, Nq, 2] = (maximum, sum) then [chunk, B, Nq, H * 32] =
    dQ unscaled) and combined in chunk order.  stats_out: as attention_bwd_long's."""
    need = attention_bwd_wide_scratch(B, H, Nq, Nk, head_dim)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.float32, device=q.device)
    _need(scratch, torch.float32, "scratch")
    if not scratch.is_contiguous():
        raise ValueError("attention_bwd_wide: scratch must be contiguous")
    return _attention_bwd("attention_bwd_wide", "ldt_attention_bwd_wide", q, k, v, o, do, B, H, (Nq, Nk), head_dim,
                          lambda Cc: (_bf16_rows_out(dq_out, B * Nq, Cc, q.device, "attention_bwd_wide: dq_out"),)
                          + _bf16_rows_out(dkv_out, B * Nk, 2 * Cc, q.device, "attention_bwd_wide: dkv_out").split(Cc, 1),
                          extra=lambda Cc: (_p(scratch), scratch.numel()), stats_out=stats_out)


def reparam_kl_bwd(post, noise, d_eps, kl_scale, lo, hi):
    """Backward of `reparam_kl`'s draw and of kl_scale * kl.sum() (ldt_reparam_kl_bwd): post fp32 [rows, 2z] = mu | logvar as stored, noise
    [rows, z], d_eps [rows, z] (strided slice ok) -> dpost fp32 [rows, 2z] = dmu | dlogvar, exactly 0 where logvar is outside [lo, hi]."""
    _need(post, torch.float32, "post"); _need(noise, torch.float32, "noise"); _need(d_eps, torch.float32, "d_eps")
    if post.dim() != 2 or post.shape[1] % 2:
        raise ValueError("reparam_kl_bwd: post %s is not [rows, 2z]" % (tuple(post.shape),))
    rows, z = post.shape[0], post.shape[1] // 2
    if not (post.is_contiguous() and noise.is_contiguous() and noise.numel() == rows * z and tuple(d_eps.shape) == (rows, z)
            and d_eps.stride(1) == 1 and d_eps.stride(0) >= z):
        raise ValueError("reparam_kl_bwd: post [rows, 2z] and noise [rows, z] contiguous, d_eps [rows, z] with unit column stride")
    out = torch.empty_like(post)
    check(lib().ldt_reparam_kl_bwd(_p(post), _p(noise), _p(d_eps), d_eps.stride(0), float(kl_scale), _p(out), rows, z, float(lo), float(hi),
                                   stream_ptr()), "ldt_reparam_kl_bwd")
    return out


def chamfer_nn(x1, x2):
    """x1 [B, n, 3], x2 [B, m, 3] fp32 -> (d1 [B, n], idx1 [B, n] int32, d2 [B, m], idx2 [B, m] int32): squared nearest-neighbour
    distances both ways (bit-equal to chamfer(x1, x2)'s dr and dl) with the lowest index that attains each."""
    _need(x1, torch.float32, "x1"); _need(x2, torch.float32, "x2")
    if x1.dim() != 3 or x2.dim() != 3 or x1.shape[2] != 3 or x2.shape[2] != 3 or x1.shape[0] != x2.shape[0]:
        raise ValueError("chamfer_nn: x1 %s, x2 %s are not [B, n, 3] and [B, m, 3]" % (tuple(x1.shape), tuple(x2.shape)))
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    d1, d2 = torch.empty((B, n), dtype=torch.float32, device=x1.device), torch.empty((B, m), dtype=torch.float32, device=x1.device)
    i1, i2 = torch.empty((B, n), dtype=torch.int32, device=x1.device), torch.empty((B, m), dtype=torch.int32, device=x1.device)
    check(lib().ldt_chamfer_nn(_p(x1), _p(x2), B, n, m, _p(d1), _p(i1), _p(d2), _p(i2), stream_ptr()), "ldt_chamfer_nn")
    return d1, i1, d2, i2


def _cd_type(type):
    if type not in _lib.CD_TYPES:
        raise ValueError("cd_loss: type %r is neither 'l1' nor 'l2'" % (type,))
    return _lib.CD_TYPES[type]


def cd_loss(d1, d2, type="l1", out=None):
    """fp32 [3] on the device = (loss, term1, term2) of CD_loss over chamfer_nn's distances: 'l1' mean sqrt(d1) + mean sqrt(d2), 'l2'
    mean d1 + mean d2.  Float64 partials in index order."""
    t = _cd_type(type)
    _need(d1, torch.float32, "d1"); _need(d2, torch.float32, "d2")
    if not (d1.is_contiguous() and d2.is_contiguous()):
        raise ValueError("cd_loss: d1 and d2 must be contiguous")
    if out is None:
        out = torch.empty((3,), dtype=torch.float32, device=d1.device)
    _need(out, torch.float32, "out")
    check(lib().ldt_cd_loss(_p(d1), d1.numel(), _p(d2), d2.numel(), t, _p(out), stream_ptr()), "ldt_cd_loss")
    return out


def cd_loss_bwd(x1, x2, idx1, idx2, type="l1", upstream=1.0):
    """fp32 [B, n, 3]: upstream * d cd_loss / d x1 (the estimated cloud) from chamfer_nn's indices.  A pair at distance 0 contributes 0."""
    _need(x1, torch.float32, "x1"); _need(x2, torch.float32, "x2"); _need(idx1, torch.int32, "idx1"); _need(idx2, torch.int32, "idx2")
    t = _cd_type(type)
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    if tuple(idx1.shape) != (B, n) or tuple(idx2.shape) != (B, m) or x2.shape[0] != B or not (idx1.is_contiguous() and idx2.is_contiguous()):
        raise ValueError("cd_loss_bwd: idx1 %s, idx2 %s for x1 %s, x2 %s" % (tuple(idx1.shape), tuple(idx2.shape), tuple(x1.shape), tuple(x2.shape)))
    out = torch.empty_like(x1)
    check(lib().ldt_cd_loss_bwd(_p(x1), _p(x2), _p(idx1), _p(idx2), B, n, m, t, float(upstream), _p(out), stream_ptr()), "ldt_cd_loss_bwd")
    return out


def prior_row_map(keep):
    """The `src` of rows_gather_sum for a set that starts from the kept prior rows packed to the front (InitialSet under a keep mask,
    Compressor/layers.py:34-37): keep bool [B, R] (True = sample b holds prior row r) -> int32 [B, R], the running count of kept rows before
    r where kept, -1 elsewhere.  Index bookkeeping on whichever device `keep` lives on; without a mask src[b][r] = r."""
    keep = keep.to(torch.bool)
    pos = keep.to(torch.int32).cumsum(1, dtype=torch.int32) - 1
    return torch.where(keep, pos, torch.full_like(pos, -1)).contiguous()


def rows_gather_sum(dy, src, N):
    """fp32 [R, C]: row r = the sum over the samples b with src[b, r] >= 0, in the order of b, of dy[b * N + src[b, r]].  dy fp32 [B * N, C]
    row-major, src int32 [B, R] (-1 = sample b does not hold row r)."""
    _need(dy, torch.float32, "dy"); _rowmajor(dy, "dy"); _need(src, torch.int32, "src")
    B, R = src.shape
    if dy.dim() != 2 or dy.shape[0] != B * N or not src.is_contiguous():
        raise ValueError("rows_gather_sum: dy %s is not [B * N, C] for contiguous src %s, N %d" % (tuple(dy.shape), tuple(src.shape), N))
    out = torch.empty((R, dy.shape[1]), dtype=torch.float32, device=dy.device)
    check(lib().ldt_rows_gather_sum(_p(dy), dy.stride(0), _p(src), B, int(N), R, dy.shape[1], _p(out), stream_ptr()), "ldt_rows_gather_sum")
    return out


def sumsq(x, max_norm=0.0, scratch=None, out=None):
    """fp32 [3] on the device = (sum x^2, its root, min(1, max_norm / (root + 1e-6))) of a flat fp32 buffer: clip_grad_norm_'s total norm
    and factor without a host synchronisation.  Two stages, fixed order."""
    _need(x, torch.float32, "x")
    if not x.is_contiguous():
        raise ValueError("sumsq: x must be contiguous")
    if scratch is None:
        scratch = torch.empty((_lib.ODE_SUMSQ_SCRATCH,), dtype=torch.float64, device=x.device)
    if out is None:
        out = torch.empty((3,), dtype=torch.float32, device=x.device)
    _need(scratch, torch.float64, "scratch"); _need(out, torch.float32, "out")
    check(lib().ldt_sumsq(_p(x), x.numel(), _p(scratch), scratch.numel(), float(max_norm or 0.0), _p(out), stream_ptr()), "ldt_sumsq")
    return out


def adam_ema_step_(param, grad, exp_avg, exp_avg_sq, ema, step, lr, beta1, beta2, eps, weight_decay, ema_decay, ema_init, clip_factor=None):
    """One fused torch-order Adam update + reference EMA over flat fp32 buffers, in place.  step: the step being taken (from 1);
    clip_factor: a device float (sumsq(...)[2:]) or None."""
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (ema, "ema"), (clip_factor, "clip_factor")):
        _need(t, torch.float32, nm)
        if t is not None and not t.is_contiguous():
            raise ValueError("adam_ema_step_: %s must be contiguous" % nm)
    n = param.numel()
    if any(t is not None and t.numel() != n for t in (grad, exp_avg, exp_avg_sq, ema)):
        raise ValueError("adam_ema_step_: the flat buffers must hold %d elements each" % n)
    check(lib().ldt_adam_ema_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(ema), n, float(lr), float(beta1), float(beta2), float(eps),
                                  float(weight_decay), int(step), float(ema_decay), int(bool(ema_init)), _p(clip_factor), stream_ptr()),
          "ldt_adam_ema_step")
