// Device half of the probability-flow ODE sampler (`sample_mode: continuous`, diffusion/diffusion_continuous.py:88-131): the
// Dormand-Prince 5(4) arithmetic scipy's RK45 does on the host between two Score evaluations (scipy/integrate/_ivp/rk.py
// rk_step / _step_impl, common.py select_initial_step), on the flattened state as scipy holds it: y and the stage derivatives
// K[0..6] are float64 [n].  Three HBM-streaming passes over a few MB each, written like samplers.hip for determinism rather
// than speed: fixed operation and reduction order, no float atomics, no FMA contraction, grid-stride with a capped grid.
// The step controller itself (accept / reject, the next step size) stays on the host: ldt_amd/ode.py.
#include "../../include/ldt_hip.h"
#include "kernels.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));

#define ODE_THREADS 256
#define ODE_MAX_GRID 1024          // = LDT_ODE_SUMSQ_SCRATCH: one fp64 partial per workgroup of the norm's first stage

__host__ __device__ static inline bool ode_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// ------------------------------------------------------------------------------------------------
// y_s = y + h * (((a0 K0 + a1 K1) + a2 K2) + ...), 1..6 terms left to right in fp64; x_s = (float)y_s is the Score's input.
struct OdeStageArgs { const double* y; const double* k[6]; double a[6]; double h; double* y_out; float* x_out; long npair; };
template <int NT>
__global__ __launch_bounds__(ODE_THREADS) void ode_stage_kernel(const OdeStageArgs g) {
    for (long i = blockIdx.x * (long)ODE_THREADS + threadIdx.x; i < g.npair; i += (long)gridDim.x * ODE_THREADS) {
        const f64x2 yv = *reinterpret_cast<const f64x2*>(g.y + 2 * i);
        f64x2 kv[NT];
#pragma unroll
        for (int s = 0; s < NT; ++s) kv[s] = *reinterpret_cast<const f64x2*>(g.k[s] + 2 * i);
        f64x2 o;
        f32x2 x;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double acc = g.a[0] * kv[0][j];
#pragma unroll
                for (int s = 1; s < NT; ++s) {
                    const double term = g.a[s] * kv[s][j];
                    acc = acc + term;
                }
                const double dy = g.h * acc;
                o[j] = yv[j] + dy;
                x[j] = (float)o[j];
            }
        }
        *reinterpret_cast<f64x2*>(g.y_out + 2 * i) = o;
        *reinterpret_cast<f32x2*>(g.x_out + 2 * i) = x;
    }
}

extern "C" int ldt_ode_stage(const double* y, const double* k0, const double* k1, const double* k2, const double* k3, const double* k4,
                             const double* k5, double a0, double a1, double a2, double a3, double a4, double a5, int32_t nterms, double h,
                             double* y_out, float* x_out, int64_t n, void* stream) {
    LDT_REQUIRE(nterms >= 1 && nterms <= 6, LDT_EARG, "ode_stage: nterms=%d must be 1..6", nterms);
    OdeStageArgs g{y, {k0, k1, k2, k3, k4, k5}, {a0, a1, a2, a3, a4, a5}, h, y_out, x_out, 0};
    LDT_REQUIRE(y && y_out && x_out, LDT_EARG, "ode_stage: null pointer");
    for (int s = 0; s < nterms; ++s) LDT_REQUIRE(g.k[s], LDT_EARG, "ode_stage: null pointer (K%d of %d terms)", s, nterms);
    LDT_REQUIRE(n > 0 && n % 2 == 0, LDT_ESHAPE, "ode_stage: n=%ld must be a positive multiple of 2 (two fp64 per 16-byte access)", (long)n);
    bool al = ldt_aligned16(y) && ldt_aligned16(y_out) && ode_aligned8(x_out);
    for (int s = 0; s < nterms; ++s) al = al && ldt_aligned16(g.k[s]);
    LDT_REQUIRE(al, LDT_EALIGN, "ode_stage: fp64 buffers must be 16-byte aligned, x_out 8-byte aligned");
    g.npair = n / 2;
    const dim3 grid(ldt_grid_1d(g.npair, ODE_THREADS, ODE_MAX_GRID)), block(ODE_THREADS);
    hipStream_t s = ldt_stream(stream);
    switch (nterms) {
        case 1: hipLaunchKernelGGL(ode_stage_kernel<1>, grid, block, 0, s, g); break;
        case 2: hipLaunchKernelGGL(ode_stage_kernel<2>, grid, block, 0, s, g); break;
        case 3: hipLaunchKernelGGL(ode_stage_kernel<3>, grid, block, 0, s, g); break;
        case 4: hipLaunchKernelGGL(ode_stage_kernel<4>, grid, block, 0, s, g); break;
        case 5: hipLaunchKernelGGL(ode_stage_kernel<5>, grid, block, 0, s, g); break;
        default: hipLaunchKernelGGL(ode_stage_kernel<6>, grid, block, 0, s, g); break;
    }
    return ldt_check_launch("ode_stage");
}

// ------------------------------------------------------------------------------------------------
// K = double(-(f x - (0.5 g2) score)), score = -params / sd: Trainer.score_fn followed by fun() of
// DiffusionBase.sample_model_ode, one fp32 operation per line in their order, then widened.  f, g2, sd are batch-uniform
// (every sample sits at the same t) and come from the host's SDE object.  is_score: `p` already holds the score.
__global__ __launch_bounds__(ODE_THREADS) void ode_rhs_kernel(const float* __restrict__ x, const float* __restrict__ p, int is_score, float f,
                                                              float hg2, float sd, double* __restrict__ k_out, long npair) {
    for (long i = blockIdx.x * (long)ODE_THREADS + threadIdx.x; i < npair; i += (long)gridDim.x * ODE_THREADS) {
        const f32x2 xv = *reinterpret_cast<const f32x2*>(x + 2 * i);
        const f32x2 pv = *reinterpret_cast<const f32x2*>(p + 2 * i);
        f64x2 o;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float score = is_score ? pv[j] : -pv[j] / sd;
                const float a = f * xv[j];
                const float b = hg2 * score;
                const float dx = a - b;
                o[j] = (double)(-dx);
            }
        }
        *reinterpret_cast<f64x2*>(k_out + 2 * i) = o;
    }
}

extern "C" int ldt_ode_rhs(const float* x, const float* p, int32_t is_score, float f, float g2, float sd, double* k_out, int64_t n, void* stream) {
    LDT_REQUIRE(x && p && k_out, LDT_EARG, "ode_rhs: null pointer");
    LDT_REQUIRE(is_score || sd > 0.f, LDT_EARG, "ode_rhs: sd=%g must be positive", (double)sd);
    LDT_REQUIRE(n > 0 && n % 2 == 0, LDT_ESHAPE, "ode_rhs: n=%ld must be a positive multiple of 2 (two fp64 per 16-byte access)", (long)n);
    LDT_REQUIRE(ode_aligned8(x) && ode_aligned8(p) && ldt_aligned16(k_out), LDT_EALIGN, "ode_rhs: x / p must be 8-byte, k_out 16-byte aligned");
    const float hg2 = 0.5f * g2;                               // `0.5 * self.g2(t)` (exact)
    hipLaunchKernelGGL(ode_rhs_kernel, dim3(ldt_grid_1d(n / 2, ODE_THREADS, ODE_MAX_GRID)), dim3(ODE_THREADS), 0, ldt_stream(stream), x, p, (int)is_score, f,
                       hg2, sd, k_out, (long)(n / 2));
    return ldt_check_launch("ode_rhs");
}

// ------------------------------------------------------------------------------------------------
// *out = sum_i ((sum_j c_j v_j[i]) / (atol + rtol max(|ya[i]|, |yb[i]|)))^2 — the square of scipy's norm(err / scale) — in two
// stages: every workgroup's partial (thread-serial, then xor-shuffle within each wave, then the four waves left to right) goes to
// scratch[blockIdx], one workgroup adds the partials the same way.  The order is a function of n alone: launches repeat bit for bit.
__device__ __forceinline__ double ode_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double ode_block_sum(double acc) {
    acc = ode_wave_sum(acc);
    __shared__ double part[ODE_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}
struct OdeNormArgs { const double* v[7]; double c[7]; const double* ya; const double* yb; double atol, rtol; double* partial; long npair; };
template <int NV>
__global__ __launch_bounds__(ODE_THREADS) void ode_sumsq_partial_kernel(const OdeNormArgs g) {
    double acc = 0.0;
    for (long i = blockIdx.x * (long)ODE_THREADS + threadIdx.x; i < g.npair; i += (long)gridDim.x * ODE_THREADS) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(g.ya + 2 * i);
        const f64x2 b = *reinterpret_cast<const f64x2*>(g.yb + 2 * i);
        f64x2 vv[NV];
#pragma unroll
        for (int s = 0; s < NV; ++s) vv[s] = *reinterpret_cast<const f64x2*>(g.v[s] + 2 * i);
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double e = g.c[0] * vv[0][j];
#pragma unroll
                for (int s = 1; s < NV; ++s) {
                    const double term = g.c[s] * vv[s][j];
                    e = e + term;
                }
                const double m = fmax(fabs(a[j]), fabs(b[j]));
                const double rm = g.rtol * m;
                const double scale = g.atol + rm;
                const double q = e / scale;
                const double q2 = q * q;
                acc = acc + q2;
            }
        }
    }
    const double tot = ode_block_sum(acc);
    if (threadIdx.x == 0) g.partial[blockIdx.x] = tot;
}
__global__ __launch_bounds__(ODE_THREADS) void ode_sumsq_final_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += ODE_THREADS) acc += partial[i];
    const double tot = ode_block_sum(acc);
    if (threadIdx.x == 0) *out = tot;
}

extern "C" int ldt_ode_scaled_sumsq(const double* v0, const double* v1, const double* v2, const double* v3, const double* v4, const double* v5,
                                    const double* v6, double c0, double c1, double c2, double c3, double c4, double c5, double c6, int32_t nvec,
                                    const double* ya, const double* yb, double atol, double rtol, double* scratch, int32_t scratch_len,
                                    double* out, int64_t n, void* stream) {
    LDT_REQUIRE(nvec >= 1 && nvec <= 7, LDT_EARG, "ode_scaled_sumsq: nvec=%d must be 1..7", nvec);
    OdeNormArgs g{{v0, v1, v2, v3, v4, v5, v6}, {c0, c1, c2, c3, c4, c5, c6}, ya, yb, atol, rtol, scratch, 0};
    LDT_REQUIRE(ya && yb && scratch && out, LDT_EARG, "ode_scaled_sumsq: null pointer");
    for (int s = 0; s < nvec; ++s) LDT_REQUIRE(g.v[s], LDT_EARG, "ode_scaled_sumsq: null pointer (v%d of %d vectors)", s, nvec);
    LDT_REQUIRE(scratch_len >= 1, LDT_EARG, "ode_scaled_sumsq: scratch_len=%d (one fp64 per workgroup, LDT_ODE_SUMSQ_SCRATCH = %d always suffice)",
                scratch_len, ODE_MAX_GRID);
    LDT_REQUIRE(atol >= 0.0 && rtol >= 0.0 && (atol > 0.0 || rtol > 0.0), LDT_EARG, "ode_scaled_sumsq: atol=%g rtol=%g", atol, rtol);
    LDT_REQUIRE(n > 0 && n % 2 == 0, LDT_ESHAPE, "ode_scaled_sumsq: n=%ld must be a positive multiple of 2 (two fp64 per 16-byte access)", (long)n);
    bool al = ldt_aligned16(ya) && ldt_aligned16(yb) && ode_aligned8(scratch) && ode_aligned8(out);
    for (int s = 0; s < nvec; ++s) al = al && ldt_aligned16(g.v[s]);
    LDT_REQUIRE(al, LDT_EALIGN, "ode_scaled_sumsq: fp64 vectors must be 16-byte aligned, scratch / out 8-byte aligned");
    g.npair = n / 2;
    unsigned blocks = ldt_grid_1d(g.npair, ODE_THREADS, ODE_MAX_GRID);
    if (blocks > (unsigned)scratch_len) blocks = (unsigned)scratch_len;
    const dim3 grid(blocks), block(ODE_THREADS);
    hipStream_t s = ldt_stream(stream);
    switch (nvec) {
        case 1: hipLaunchKernelGGL(ode_sumsq_partial_kernel<1>, grid, block, 0, s, g); break;
        case 2: hipLaunchKernelGGL(ode_sumsq_partial_kernel<2>, grid, block, 0, s, g); break;
        case 3: hipLaunchKernelGGL(ode_sumsq_partial_kernel<3>, grid, block, 0, s, g); break;
        case 4: hipLaunchKernelGGL(ode_sumsq_partial_kernel<4>, grid, block, 0, s, g); break;
        case 5: hipLaunchKernelGGL(ode_sumsq_partial_kernel<5>, grid, block, 0, s, g); break;
        case 6: hipLaunchKernelGGL(ode_sumsq_partial_kernel<6>, grid, block, 0, s, g); break;
        default: hipLaunchKernelGGL(ode_sumsq_partial_kernel<7>, grid, block, 0, s, g); break;
    }
    hipLaunchKernelGGL(ode_sumsq_final_kernel, dim3(1), block, 0, s, (const double*)scratch, (int)blocks, out);
    return ldt_check_launch("ode_scaled_sumsq");
}
