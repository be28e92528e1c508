// The optimizer half of a Score training step (trainer/Latent_SDE_Trainer.py:138-140; gfx950): the global gradient norm with
// clip_grad_norm_'s factor, and one fused Adam + EMA update over the flat fp32 parameter buffer.
//   ldt_sumsq           two stages, fixed order, float64 partials (as ldt_nelbo_terms / ldt_ode_scaled_sumsq): repeats bit for bit.
//   ldt_adam_ema_step   torch.optim.Adam's single-tensor update (its formulas in its order, each in the fewest-roundings form), then the
//                       reference's EMA (tools/utils.py:34-71).
// The clip factor is read from device memory, so a step never waits for the host.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define SUMSQ_WG 256

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// valid in thread 0
__device__ __forceinline__ double block_sum_f64_fixed(double v) {
    __shared__ double part[SUMSQ_WG / LDT_WAVE];
    v = wave_sum_f64(v);
    if ((threadIdx.x & (LDT_WAVE - 1)) == 0) part[threadIdx.x / LDT_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SUMSQ_WG / LDT_WAVE; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(SUMSQ_WG) void sumsq_partial_kernel(const float* __restrict__ x, long n, double* __restrict__ scratch) {
    double acc = 0.0;
    for (long i = blockIdx.x * (long)SUMSQ_WG + threadIdx.x; i < n; i += (long)gridDim.x * SUMSQ_WG) {
        const double v = (double)x[i];
        acc += v * v;
    }
    const double s = block_sum_f64_fixed(acc);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}
// out = {sum of squares, its root, min(1, max_norm / (root + 1e-6))}: total_norm and clip_coef_clamped of torch.nn.utils.clip_grad_norm_
__global__ __launch_bounds__(SUMSQ_WG) void sumsq_final_kernel(const double* __restrict__ scratch, int parts, float max_norm, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < parts; i += SUMSQ_WG) acc += scratch[i];
    const double s = block_sum_f64_fixed(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        out[0] = (float)s;
        out[1] = norm;
        out[2] = max_norm > 0.f ? fminf(max_norm / (norm + 1e-6f), 1.f) : 1.f;
    }
}

extern "C" int ldt_sumsq(const float* x, int64_t n, double* scratch, int32_t scratch_len, float max_norm, float* out, void* stream) {
    LDT_REQUIRE(x && scratch && out, LDT_EARG, "sumsq: null pointer");
    LDT_REQUIRE(n > 0 && scratch_len > 0, LDT_ESHAPE, "sumsq: n %ld, scratch_len %d", (long)n, scratch_len);
    hipStream_t s = ldt_stream(stream);
    long parts = (n + SUMSQ_WG - 1) / SUMSQ_WG;
    if (parts > scratch_len) parts = scratch_len;
    if (parts > LDT_ODE_SUMSQ_SCRATCH) parts = LDT_ODE_SUMSQ_SCRATCH;
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)parts), dim3(SUMSQ_WG), 0, s, x, (long)n, scratch);
    int rc = ldt_check_launch("sumsq");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(SUMSQ_WG), 0, s, scratch, (int)parts, max_norm, out);
    return ldt_check_launch("sumsq (final)");
}

// torch/optim/adam.py _single_tensor_adam (amsgrad False, maximize False, coupled weight decay) after clip_grad_norm_'s grad.mul_(coef):
//     g = g * coef;  g = g + wd * p  (wd != 0);  m.lerp_(g, 1 - b1);  v.mul_(b2).addcmul_(g, g, value = 1 - b2);
//     denom = (v.sqrt() / sqrt(1 - b2^t)).add_(eps);  p.addcdiv_(m, denom, value = -lr / (1 - b1^t))
// then tools/utils.py:49-62:  ema = p.clone() on the first step, and ema.mul_(d).add_(p, alpha = 1 - d) on every step (the first included).
// Same formulas in the same order, each in the form with the fewest roundings at the magnitude of the stored value (contraction is off: the
// fused multiply-adds below are spelled out):  g + wd p in float64, rounded once (the sum cancels where the two terms oppose);
// m = fma(w, g - m, m) (what at::lerp's CPU kernel issues);  v = fma(1 - b2, g g - v, v), the lerp form of v b2 + (1 - b2) g g: the fp32
// constant b2 is itself 2^-24 off, and v b2 would carry that at the magnitude of v, where this form carries it at the magnitude of the change;
// p = p + (s m) / denom (addcdiv's `value * t1 / t2`);  ema = fma(1 - d, p - ema, ema), the lerp form of ema d + (1 - d) p: its error is
// 2^-24 |ema| + O(2^-24 |ema - p|) instead of two roundings at |ema| — and ema == p exactly after a parameter's first step.  sqrtf and the
// divisions are the correctly rounded ones (no fast-math).
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, long n, float w1, float w2, float eps, double wd,
                                                       float neg_step_size, float bc2_sqrt, float wd_ema, int ema_init,
                                                       const float* __restrict__ clip_factor) {
#pragma clang fp contract(off)
    const float coef = clip_factor ? *clip_factor : 1.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float pi = p[i];
        float gi = g[i] * coef;
        if (clip_factor) g[i] = gi;                                   // clip_grad_norm_ scales p.grad in place
        if (wd != 0.0) gi = (float)((double)gi + wd * (double)pi);
        float mi = m[i];
        mi = w1 < 0.5f ? fmaf(w1, gi - mi, mi) : fmaf(w1 - 1.f, gi - mi, gi);   // at::lerp's two forms
        const float v0 = v[i];
        const float vi = fmaf(w2, gi * gi - v0, v0);
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi = pi + (neg_step_size * mi) / denom;
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (ema) {
            const float e = ema_init ? pi : ema[i];
            ema[i] = fmaf(wd_ema, pi - e, e);
        }
    }
}

extern "C" int ldt_adam_ema_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, int32_t step, double ema_decay, int32_t ema_init,
                                 const float* clip_factor, void* stream) {
    LDT_REQUIRE(param && grad && exp_avg && exp_avg_sq, LDT_EARG, "adam_ema_step: null pointer");
    LDT_REQUIRE(n > 0 && step >= 1, LDT_ESHAPE, "adam_ema_step: n %ld, step %d (the step that is being taken, counted from 1)", (long)n, step);
    // the scalars are Python floats upstream: formed in double, rounded to fp32 where torch's kernels take them
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float neg_step_size = (float)(-(lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_ema_kernel, dim3(ldt_grid_1d(n, 256, 4096)), dim3(256), 0, ldt_stream(stream), param, grad, exp_avg, exp_avg_sq,
                       ema, (long)n, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, weight_decay, neg_step_size, bc2_sqrt,
                       (float)(1.0 - ema_decay), ema_init, clip_factor);
    return ldt_check_launch("adam_ema_step");
}
