// Device ops of the samplers around the Score forward.  All are HBM-streaming passes over the latents [B][tokens*z] fp32 — a few MB, far
// below the Score forward they sit next to — written for determinism (fixed reduction order, no atomics) rather than speed:
//   sampler_step, advance_step    the fused predictor update with in-kernel Philox noise and the device-side step counter (ldt_sampler_step,
//                                 ldt_sampler_step_traj; the sampling loop of api.hip)
//   philox_normal                 the stand-alone normal fill on the same Philox stream (ldt_philox_normal)
//   batch_norms, norm_sum, langevin_coef    LangevinCorrector (diffusion/diffusion_continuous.py:193-210: ldt_batch_norm_sum, ldt_langevin_coef)
//   pndm_transfer, lincomb4       PNDM (:260-316: ldt_pndm_transfer, ldt_lincomb4)
//   vpsde_score, sde_score        score = -params / sqrt(var(t)) per SDE family (ldt_vpsde_score, ldt_sde_score)
#include "../../include/ldt_hip.h"
#include "kernels.h"

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller (philox4x32_10, box_muller): common.h — shared with the held-out-loss kernels (eval_loss.hip).

// Fused predictor update (one pass over the latents):
//   mode 0 (ancestral, exact op order of diffusion_continuous.py:152-162 + Latent_SDE_Trainer.py:57-61):
//       score = -params / std ; x_mean = (x + beta*score) / sqrt(1-beta) ; x = x_mean + sqrt(beta)*z
//       coef[step] = {beta, std, sqrt(1-beta), sqrt(beta)}   (host fp32 tables, SURVEY hard part 4)
//   mode 1 (folded; reversediffusion / eulermaruyama / ddim, :141-191):
//       x_mean = A*x + Bc*params ; x = x_mean + Cc*z        coef[step] = {A, Bc, Cc, 0}
// z comes from `noise` (parity mode: injected CPU draws) or from Philox keyed by
// (seed, stream id = step*philox_mul + philox_add, global element index) so that a sample's noise does not depend on how the batch is sharded.
__global__ __launch_bounds__(256) void sampler_step_kernel(const StepArgs a) {
    const int step = a.step_ptr ? *a.step_ptr : a.step_host;
    const f32x4 cf = *reinterpret_cast<const f32x4*>(a.coef + 4L * step);
    const float* nz = a.noise ? a.noise + (long)step * a.noise_step_stride : nullptr;
    const long nvec = a.n / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a.x + 4 * i);
        const f32x4 p = *reinterpret_cast<const f32x4*>(a.params + 4 * i);
        f32x4 z;
        if (nz) {
            z = *reinterpret_cast<const f32x4*>(nz + 4 * i);
        } else {
            const uint64_t e = (uint64_t)(a.elem_offset / 4 + i);
            uint32_t c[4] = {(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)(step * a.philox_mul + a.philox_add), 0x4C445421u};
            philox4x32_10(c, a.seed_lo, a.seed_hi);
            float z0, z1, z2, z3;
            box_muller(c[0], c[1], z0, z1);
            box_muller(c[2], c[3], z2, z3);
            z = (f32x4){z0, z1, z2, z3};
        }
        f32x4 xm, xn;
        {
#pragma clang fp contract(off)      // the reference's separate mul/add/div roundings, no FMA (HIP's __f*_rn are plain ops)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (a.mode == 0) {
                    const float score = -p[j] / cf[1];
                    const float bs = cf[0] * score;
                    const float num = x[j] + bs;
                    xm[j] = num / cf[2];
                } else {
                    const float ax = cf[0] * x[j];
                    const float bp = cf[1] * p[j];
                    xm[j] = ax + bp;
                }
                const float cz = (a.mode == 0) ? cf[3] : cf[2];
                const float nz_ = cz * z[j];
                xn[j] = xm[j] + nz_;
            }
        }
        *reinterpret_cast<f32x4*>(a.x_out + 4 * i) = xn;
        if (a.traj) *reinterpret_cast<f32x4*>(a.traj + (long)step * a.n + 4 * i) = xn;
        if (a.x_mean_out) *reinterpret_cast<f32x4*>(a.x_mean_out + 4 * i) = xm;
    }
}

__global__ void advance_step_kernel(int* step_ptr) { if (threadIdx.x == 0 && blockIdx.x == 0) *step_ptr += 1; }

int ldt_sampler_step_launch(const StepArgs* a, hipStream_t s) {
    LDT_REQUIRE(a->n > 0 && a->n % 4 == 0 && a->elem_offset % 4 == 0, LDT_ESHAPE, "sampler_step: n and elem_offset must be multiples of 4 (n=%ld)", a->n);
    LDT_REQUIRE(a->x && a->params && a->x_out && a->coef, LDT_EARG, "sampler_step: null pointer");
    LDT_REQUIRE(ldt_aligned16(a->x) && ldt_aligned16(a->params) && ldt_aligned16(a->x_out) && ldt_aligned16(a->coef) &&
                (!a->noise || ldt_aligned16(a->noise)) && (!a->x_mean_out || ldt_aligned16(a->x_mean_out)) && a->noise_step_stride % 4 == 0,
                LDT_EALIGN, "sampler_step: buffers must be 16-byte aligned");
    LDT_REQUIRE(a->mode == 0 || a->mode == 1, LDT_EARG, "sampler_step: mode %d", a->mode);
    hipLaunchKernelGGL(sampler_step_kernel, dim3(ldt_grid_1d(a->n / 4, 256, 2048)), dim3(256), 0, s, *a);
    return ldt_check_launch("sampler_step");
}
int ldt_advance_step_launch(int* step_ptr, hipStream_t s) {
    hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(64), 0, s, step_ptr);
    return ldt_check_launch("advance_step");
}
extern "C" int ldt_sampler_step(const float* x, const float* params, const float* noise, int64_t noise_step_stride,
                                float* x_out, float* x_mean_out, const float* coef, const int32_t* step_ptr,
                                int32_t step_host, int32_t mode, int64_t n, int64_t elem_offset, uint64_t seed,
                                int32_t philox_mul, int32_t philox_add, void* stream) {
    StepArgs a{x, params, noise, x_out, x_mean_out, coef, step_ptr, step_host, mode, n, elem_offset, noise_step_stride,
               (uint32_t)seed, (uint32_t)(seed >> 32), philox_mul, philox_add};
    return ldt_sampler_step_launch(&a, ldt_stream(stream));
}
extern "C" int ldt_sampler_step_traj(const float* x, const float* params, const float* noise, int64_t noise_step_stride,
                                     float* x_out, float* x_mean_out, float* traj, const float* coef, const int32_t* step_ptr,
                                     int32_t step_host, int32_t mode, int64_t n, int64_t elem_offset, uint64_t seed,
                                     int32_t philox_mul, int32_t philox_add, void* stream) {
    LDT_REQUIRE(!traj || ldt_aligned16(traj), LDT_EALIGN, "sampler_step_traj: traj must be 16-byte aligned");
    StepArgs a{x, params, noise, x_out, x_mean_out, coef, step_ptr, step_host, mode, n, elem_offset, noise_step_stride,
               (uint32_t)seed, (uint32_t)(seed >> 32), philox_mul, philox_add, traj};
    return ldt_sampler_step_launch(&a, ldt_stream(stream));
}

// standalone Philox normal fill (same stream as the fused step; used by tests and Compressor.sample(given_eps=None))
__global__ void philox_normal_kernel(float* out, long n, long elem_offset, int step, uint32_t k0, uint32_t k1) {
    const long nvec = n / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        const uint64_t e = (uint64_t)(elem_offset / 4 + i);
        uint32_t c[4] = {(uint32_t)e, (uint32_t)(e >> 32), (uint32_t)step, 0x4C445421u};
        philox4x32_10(c, k0, k1);
        float z0, z1, z2, z3;
        box_muller(c[0], c[1], z0, z1);
        box_muller(c[2], c[3], z2, z3);
        *reinterpret_cast<f32x4*>(out + 4 * i) = (f32x4){z0, z1, z2, z3};
    }
}
extern "C" int ldt_philox_normal(float* out, int64_t n, int64_t elem_offset, int32_t step, uint64_t seed, void* stream) {
    LDT_REQUIRE(out, LDT_EARG, "philox_normal: null pointer");
    LDT_REQUIRE(n > 0 && n % 4 == 0 && elem_offset % 4 == 0 && ldt_aligned16(out), LDT_ESHAPE, "philox_normal: n/offset %% 4, 16-byte aligned");
    hipLaunchKernelGGL(philox_normal_kernel, dim3(ldt_grid_1d(n / 4, 256, 2048)), dim3(256), 0, ldt_stream(stream), out, (long)n, (long)elem_offset,
                       (int)step, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ldt_check_launch("philox_normal");
}

// ------------------------------------------------------------------------------------------------
// per-sample L2 norms (torch.norm(v.reshape(B, -1), dim=-1), :204-205): one 256-thread workgroup per sample,
// 16-B loads, wave shuffle + LDS tree in a fixed order.
__global__ __launch_bounds__(256) void batch_norms_kernel(const float* __restrict__ x, long per, float* __restrict__ out) {
    const float* row = x + (long)blockIdx.x * per;
    float acc = 0.f;
    for (long i = threadIdx.x; i < per / 4; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
        acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    acc = wave_sum(acc);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf((part[0] + part[1]) + (part[2] + part[3]));
}
// sum over the batch of the per-sample norms (the numerator of .mean()): one wave, fixed order
__global__ __launch_bounds__(64) void norm_sum_kernel(const float* __restrict__ norms, int B, float* __restrict__ sum_out) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += 64) acc += norms[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *sum_out = acc;
}

extern "C" int ldt_batch_norm_sum(const float* x, int32_t B, int64_t per_sample, float* norms_scratch, float* sum_out, void* stream) {
    LDT_REQUIRE(x && norms_scratch && sum_out, LDT_EARG, "batch_norm_sum: null pointer");
    LDT_REQUIRE(B > 0 && per_sample > 0 && per_sample % 4 == 0 && ldt_aligned16(x), LDT_ESHAPE,
                "batch_norm_sum: per_sample=%ld must be a multiple of 4, x 16-byte aligned", (long)per_sample);
    hipStream_t s = ldt_stream(stream);
    hipLaunchKernelGGL(batch_norms_kernel, dim3((unsigned)B), dim3(256), 0, s, x, (long)per_sample, norms_scratch);
    hipLaunchKernelGGL(norm_sum_kernel, dim3(1), dim3(64), 0, s, norms_scratch, B, sum_out);
    return ldt_check_launch("batch_norm_sum");
}

// Langevin step size -> one coefficient row {A, B, C, 0} for ldt_sampler_step(mode 1) (x_mean = A x + B params, x = x_mean + C z):
//   grad = score = -params / std  =>  grad_norm = mean_b ||params_b|| / std ;  noise_norm = mean_b ||z_b||
//   step_size = (snr * noise_norm / grad_norm)^2 * 2 * alpha,  alpha = 1 (the reference's class test at :195 is never true)
//   x_mean = x + step_size * grad = x - (step_size / std) params ;  x = x_mean + sqrt(2 step_size) z
// sums[0] = sum_b ||params_b||, sums[1] = sum_b ||z_b|| over the WHOLE batch (all-reduced by the caller when sharded).
__global__ void langevin_coef_kernel(const float* __restrict__ sums, int n_total, float snr, float std_t, float* __restrict__ coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float grad_norm = (sums[0] / (float)n_total) / std_t;
    const float noise_norm = sums[1] / (float)n_total;
    const float r = snr * noise_norm / grad_norm;
    const float step = r * r * 2.0f;
    coef[0] = 1.0f; coef[1] = -step / std_t; coef[2] = sqrtf(step * 2.0f); coef[3] = 0.f;
}
extern "C" int ldt_langevin_coef(const float* sums, int32_t n_total, float snr, float std_t, float* coef_out, void* stream) {
    LDT_REQUIRE(sums && coef_out && n_total > 0 && std_t > 0.f, LDT_EARG, "langevin_coef: bad argument");
    hipLaunchKernelGGL(langevin_coef_kernel, dim3(1), dim3(64), 0, ldt_stream(stream), sums, n_total, snr, std_t, coef_out);
    return ldt_check_launch("langevin_coef");
}

// ------------------------------------------------------------------------------------------------
// PNDM (:260-316).  transfer(): x_next = x + d * (p * x - q * et) with the three schedule scalars of :267-271 formed by
// the host in fp32 (they are batch-uniform: every sample is at the same t); the element-wise op order is the reference's.
__global__ __launch_bounds__(256) void pndm_transfer_kernel(const float* __restrict__ x, const float* __restrict__ et, float d, float p,
                                                            float q, float* __restrict__ out, long nvec) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i);
        const f32x4 ev = *reinterpret_cast<const f32x4*>(et + 4 * i);
        f32x4 o;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = p * xv[j];
                const float b = q * ev[j];
                const float dl = d * (a - b);
                o[j] = xv[j] + dl;
            }
        }
        *reinterpret_cast<f32x4*>(out + 4 * i) = o;
    }
}
extern "C" int ldt_pndm_transfer(const float* x, const float* et, float d, float p, float q, float* out, int64_t n, void* stream) {
    LDT_REQUIRE(x && et && out, LDT_EARG, "pndm_transfer: null pointer");
    LDT_REQUIRE(n > 0 && n % 4 == 0 && ldt_aligned16(x) && ldt_aligned16(et) && ldt_aligned16(out), LDT_EALIGN,
                "pndm_transfer: n %% 4 and 16-byte aligned buffers");
    hipLaunchKernelGGL(pndm_transfer_kernel, dim3(ldt_grid_1d(n / 4, 256, 2048)), dim3(256), 0, ldt_stream(stream), x, et, d, p, q, out, n / 4);
    return ldt_check_launch("pndm_transfer");
}

// out = s * (((c0 a0 + c1 a1) + c2 a2) + c3 a3): the Runge-Kutta average (1/6)(e1 + 2 e2 + 2 e3 + e4) (:291) and the
// 4-step linear multistep combination (1/24)(55 e[-1] - 59 e[-2] + 37 e[-3] - 9 e[-4]) (:300), left to right as torch does.
struct Lin4Args { const float* a[4]; float c[4]; float s; float* out; long nvec; };
__global__ __launch_bounds__(256) void lincomb4_kernel(const Lin4Args g) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < g.nvec; i += (long)gridDim.x * 256) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(g.a[k] + 4 * i);
        f32x4 o;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t0 = g.c[0] * v[0][j];
                const float t1 = g.c[1] * v[1][j];
                const float t2 = g.c[2] * v[2][j];
                const float t3 = g.c[3] * v[3][j];
                const float acc = ((t0 + t1) + t2) + t3;
                o[j] = g.s * acc;
            }
        }
        *reinterpret_cast<f32x4*>(g.out + 4 * i) = o;
    }
}
extern "C" int ldt_lincomb4(const float* a0, const float* a1, const float* a2, const float* a3, float c0, float c1, float c2, float c3,
                            float s, float* out, int64_t n, void* stream) {
    LDT_REQUIRE(a0 && a1 && a2 && a3 && out, LDT_EARG, "lincomb4: null pointer");
    LDT_REQUIRE(n > 0 && n % 4 == 0 && ldt_aligned16(a0) && ldt_aligned16(a1) && ldt_aligned16(a2) && ldt_aligned16(a3) && ldt_aligned16(out),
                LDT_EALIGN, "lincomb4: n %% 4 and 16-byte aligned buffers");
    Lin4Args g{{a0, a1, a2, a3}, {c0, c1, c2, c3}, s, out, n / 4};
    hipLaunchKernelGGL(lincomb4_kernel, dim3(ldt_grid_1d(n / 4, 256, 2048)), dim3(256), 0, ldt_stream(stream), g);
    return ldt_check_launch("lincomb4");
}

// ------------------------------------------------------------------------------------------------
// score = -params / sqrt(var(t)) of Trainer.score_fn (trainer/Latent_SDE_Trainer.py:57-61) with var(t) of the VP-SDE
// (diffusion/diffusion_continuous.py:649-651) evaluated per sample in fp32 in the reference's op order:
//   var = 1 - (1 - sigma2_0) * exp(-beta0 t - 0.5 (beta1 - beta0) t t)
__global__ __launch_bounds__(256) void vpsde_score_kernel(const float* __restrict__ params, const float* __restrict__ t, float beta0, float beta1,
                                                          float sigma2_0, float* __restrict__ out, long per4) {
    const float tb = t[blockIdx.y];
    float sd;
    {
#pragma clang fp contract(off)
        const float a = -beta0 * tb;
        const float b = (0.5f * (beta1 - beta0)) * tb * tb;
        const float var = 1.0f - (1.0f - sigma2_0) * expf(a - b);
        sd = sqrtf(var);
    }
    const float* src = params + (long)blockIdx.y * per4 * 4;
    float* dst = out + (long)blockIdx.y * per4 * 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < per4; i += (long)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = -v[j] / sd;
        *reinterpret_cast<f32x4*>(dst + 4 * i) = o;
    }
}
extern "C" int ldt_vpsde_score(const float* params, const float* t, float beta0, float beta1, float sigma2_0, float* out, int32_t B,
                               int64_t per_sample, void* stream) {
    LDT_REQUIRE(params && t && out, LDT_EARG, "vpsde_score: null pointer");
    LDT_REQUIRE(B > 0 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0 && ldt_aligned16(params) && ldt_aligned16(out), LDT_ESHAPE,
                "vpsde_score: B=%d in [1, 65535], per_sample=%ld a multiple of 4, 16-byte aligned buffers", B, (long)per_sample);
    hipLaunchKernelGGL(vpsde_score_kernel, dim3(ldt_grid_1d(per_sample / 4, 256, 64), (unsigned)B), dim3(256), 0, ldt_stream(stream), params, t,
                       beta0, beta1, sigma2_0, out, (long)(per_sample / 4));
    return ldt_check_launch("vpsde_score");
}

// The same score for the other SDE families of diffusion/diffusion_continuous.py (make_diffusion :18-29): kind 1 = sub-VP
// (:705-707: var = (1 - e)^2 + sigma2_0 e, e = exp(-beta0 t - (beta1 - beta0) t^2 / 2); c = beta0, beta1, sigma2_0),
// kind 2 = VE and geometric (:746-747, :615-616: var = smin ratio^t - smin + sigma2_0; c = smin, ratio = smax / smin, sigma2_0),
// kind 0 = the VP form above.  fp32, the reference's op order.
__global__ __launch_bounds__(256) void sde_score_kernel(const float* __restrict__ params, const float* __restrict__ t, int kind, float c0, float c1,
                                                        float c2, float* __restrict__ out, long per4) {
    const float tb = t[blockIdx.y];
    float sd;
    {
#pragma clang fp contract(off)
        float var;
        if (kind == 2) {
            var = c0 * powf(c1, tb) - c0 + c2;
        } else {
            const float a = -c0 * tb;
            const float b = (0.5f * (c1 - c0)) * tb * tb;
            const float e = expf(a - b);
            if (kind == 1) {
                const float om = 1.0f - e;
                var = om * om + c2 * e;
            } else {
                var = 1.0f - (1.0f - c2) * e;
            }
        }
        sd = sqrtf(var);
    }
    const float* src = params + (long)blockIdx.y * per4 * 4;
    float* dst = out + (long)blockIdx.y * per4 * 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < per4; i += (long)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = -v[j] / sd;
        *reinterpret_cast<f32x4*>(dst + 4 * i) = o;
    }
}
extern "C" int ldt_sde_score(const float* params, const float* t, int32_t kind, float c0, float c1, float c2, float* out, int32_t B,
                             int64_t per_sample, void* stream) {
    LDT_REQUIRE(params && t && out, LDT_EARG, "sde_score: null pointer");
    LDT_REQUIRE(kind >= 0 && kind <= 2, LDT_EARG, "sde_score: kind=%d (0 vpsde, 1 sub_vpsde, 2 vesde / geometric_sde)", kind);
    LDT_REQUIRE(B > 0 && B <= 65535 && per_sample > 0 && per_sample % 4 == 0 && ldt_aligned16(params) && ldt_aligned16(out), LDT_ESHAPE,
                "sde_score: B=%d in [1, 65535], per_sample=%ld a multiple of 4, 16-byte aligned buffers", B, (long)per_sample);
    hipLaunchKernelGGL(sde_score_kernel, dim3(ldt_grid_1d(per_sample / 4, 256, 64), (unsigned)B), dim3(256), 0, ldt_stream(stream), params, t,
                       (int)kind, c0, c1, c2, out, (long)(per_sample / 4));
    return ldt_check_launch("sde_score");
}
