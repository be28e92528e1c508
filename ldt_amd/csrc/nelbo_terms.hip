// The two sums of the latent NELBO's KL term (trainer/Hybrid_Trainer.py:139-143), in one pass over eta, params and log q(z):
//   kl = mean(logqz - logpz),  logpz = -((eta - params)^2 * w_q(t) + c)   =>   kl = (sum logqz + sum (eta - params)^2 w_q) / n + c
//   ldt_nelbo_terms   per-sample (sum (eta - params)^2 * w[b], sum logqz) and the two sums over the batch.
// A streaming kernel over 3 x B x per_sample floats, next to a Score forward.  Written like eval_loss.hip: each term is formed with the
// reference's separate fp32 roundings (no FMA), every sum has a fixed order (per-thread strided partial -> wave shuffle -> LDS partials added
// in index order) and there are no atomics, so two runs of the same input are bit-identical.  The partials are carried in float64 — the sums
// run over 10^4..10^7 terms of mixed sign (log q(z)) and cost nothing next to the loads — and rounded to fp32 once, on the way out.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define NELBO_WG 1024                // one workgroup per sample, as ldt_dsm_loss

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// both sums over the workgroup in a fixed order; valid in thread 0
__device__ __forceinline__ void block_sum2_fixed(double& a, double& b) {
    __shared__ double part[2][NELBO_WG / LDT_WAVE];
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    if ((threadIdx.x & (LDT_WAVE - 1)) == 0) { part[0][threadIdx.x / LDT_WAVE] = a; part[1][threadIdx.x / LDT_WAVE] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int w = 0; w < (int)(blockDim.x / LDT_WAVE); ++w) { a += part[0][w]; b += part[1][w]; }
    }
}

__device__ __forceinline__ float nelbo_term(float e, float p, float w) {
#pragma clang fp contract(off)          // torch.square(eta - params) * weight_q: three roundings
    const float d = e - p;
    const float dist = d * d;
    return dist * w;
}

// stage 1: V = 4 (16-byte accesses) when per_sample % 4 == 0 and the buffers are 16-byte aligned, else 1
template <int V>
__global__ __launch_bounds__(NELBO_WG) void nelbo_sample_kernel(const float* __restrict__ eta, const float* __restrict__ params,
                                                                const float* __restrict__ logqz, const float* __restrict__ weight,
                                                                long per_sample, float* __restrict__ sample_sums) {
    const long off = (long)blockIdx.x * per_sample;
    const float* e = eta + off;
    const float* p = params + off;
    const float* q = logqz + off;
    const float w = weight ? weight[blockIdx.x] : 1.f;
    double acc_s = 0.0, acc_q = 0.0;
    if (V == 4) {
        for (long g = threadIdx.x; g < per_sample / 4; g += NELBO_WG) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(e + 4 * g);
            const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4 * g);
            const f32x4 c = *reinterpret_cast<const f32x4*>(q + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc_s += (double)nelbo_term(a[j], b[j], w);
                acc_q += (double)c[j];
            }
        }
    } else {
        for (long g = threadIdx.x; g < per_sample; g += NELBO_WG) {
            acc_s += (double)nelbo_term(e[g], p[g], w);
            acc_q += (double)q[g];
        }
    }
    block_sum2_fixed(acc_s, acc_q);
    if (threadIdx.x == 0) {
        sample_sums[2 * (long)blockIdx.x] = (float)acc_s;
        sample_sums[2 * (long)blockIdx.x + 1] = (float)acc_q;
    }
}

// stage 2: the sums over the batch of the per-sample sums, one workgroup, fixed order
__global__ __launch_bounds__(NELBO_WG) void nelbo_batch_kernel(const float* __restrict__ sample_sums, long B, float* __restrict__ batch_sums) {
    double acc_s = 0.0, acc_q = 0.0;
    for (long i = threadIdx.x; i < B; i += NELBO_WG) {
        acc_s += (double)sample_sums[2 * i];
        acc_q += (double)sample_sums[2 * i + 1];
    }
    block_sum2_fixed(acc_s, acc_q);
    if (threadIdx.x == 0) { batch_sums[0] = (float)acc_s; batch_sums[1] = (float)acc_q; }
}

extern "C" int ldt_nelbo_terms(const float* eta, const float* params, const float* logqz, const float* weight, int64_t B, int64_t per_sample,
                               float* sample_sums, float* batch_sums, void* stream) {
    LDT_REQUIRE(eta && params && logqz && sample_sums, LDT_EARG,
                "nelbo_terms: null pointer (sample_sums is the first stage's output and is required)");
    LDT_REQUIRE(B > 0 && B <= 0x7fffffffL && per_sample > 0, LDT_ESHAPE, "nelbo_terms: B %ld, per_sample %ld", (long)B, (long)per_sample);
    hipStream_t s = ldt_stream(stream);
    if (per_sample % 4 == 0 && ldt_aligned16(eta) && ldt_aligned16(params) && ldt_aligned16(logqz))
        hipLaunchKernelGGL(nelbo_sample_kernel<4>, dim3((unsigned)B), dim3(NELBO_WG), 0, s, eta, params, logqz, weight, (long)per_sample, sample_sums);
    else
        hipLaunchKernelGGL(nelbo_sample_kernel<1>, dim3((unsigned)B), dim3(NELBO_WG), 0, s, eta, params, logqz, weight, (long)per_sample, sample_sums);
    int rc = ldt_check_launch("nelbo_terms");
    if (rc != LDT_OK || !batch_sums) return rc;
    hipLaunchKernelGGL(nelbo_batch_kernel, dim3(1), dim3(NELBO_WG), 0, s, sample_sums, (long)B, batch_sums);
    return ldt_check_launch("nelbo_terms (batch)");
}
