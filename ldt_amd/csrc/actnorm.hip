// ActNorm (gfx950): z = (x - shift) * exp(-log_scale), shift and log_scale shared by the B samples (model/layers.py:103-107; the parameters
// :66-72).  actnorm_kernel is the forward (ldt_actnorm, in place); actnorm_bwd_kernel and actnorm_bwd_combine_kernel are its backward
// (ldt_actnorm_bwd).  From the gradient dz and the forward's OUTPUT z (the forward runs in place: z is what the tape holds):
//     dx[b][i] = dz[b][i] * exp(-log_scale[i]),   dshift[i] = -sum_b dx[b][i],   dlog_scale[i] = -sum_b dz[b][i] * z[b][i].
// One streaming kernel: a thread owns V columns (V = 4: 16-byte accesses; V = 1: the scalar form of the same kernel) and a contiguous run of
// rows; what it shares with the reductions of score_bwd.hip:
//   * no atomics, a fixed order: the rows of a workgroup are cut into ANB_SLICES contiguous runs, each summed in the order of b, the runs
//     added in index order; past ANB_ROWS rows (the 'set' form: per_sample = C, B T rows) every workgroup writes its partial and a second
//     kernel adds the partials in index order.  Two runs of one input give the same bits;
//   * the sums are carried in float64 and rounded to fp32 once: dx enters its sum as the fp32 value that is stored, dz * z as the exact
//     float64 product of the two fp32 factors.
#include "../../include/ldt_hip.h"
#include "kernels.h"

// forward (eval): y[b,t,c] = (x[b,t,c] - shift[t,c]) * exp(-log_scale[t,c]), in place
__global__ void actnorm_kernel(float* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ log_scale,
                               long total, long per_sample) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long j = i % per_sample;
        x[i] = (x[i] - shift[j]) * expf(-log_scale[j]);
    }
}
extern "C" int ldt_actnorm(float* x, const float* shift, const float* log_scale, int64_t B, int64_t per_sample, void* stream) {
    LDT_REQUIRE(x && shift && log_scale, LDT_EARG, "actnorm: null pointer");
    LDT_REQUIRE(B > 0 && per_sample > 0, LDT_ESHAPE, "actnorm: bad shape");
    const long total = B * per_sample;
    hipLaunchKernelGGL(actnorm_kernel, dim3(ldt_grid_1d(total, 256, 4096)), dim3(256), 0, ldt_stream(stream), x, shift, log_scale, total, (long)per_sample);
    return ldt_check_launch("actnorm");
}

#define ANB_COLS 16                 // column groups (of V columns) per workgroup
#define ANB_SLICES 16                // row runs per workgroup
#define ANB_ROWS 512                 // rows per workgroup: more rows take a second stage

template <int V> struct anb_vec;
template <> struct anb_vec<4> { typedef f32x4 type; };
template <> struct anb_vec<1> { typedef float type; };
template <int V> __device__ __forceinline__ float anb_get(const typename anb_vec<V>::type& v, int k);
template <> __device__ __forceinline__ float anb_get<4>(const f32x4& v, int k) { return v[k]; }
template <> __device__ __forceinline__ float anb_get<1>(const float& v, int) { return v; }
template <int V> __device__ __forceinline__ void anb_set(typename anb_vec<V>::type& v, int k, float x);
template <> __device__ __forceinline__ void anb_set<4>(f32x4& v, int k, float x) { v[k] = x; }
template <> __device__ __forceinline__ void anb_set<1>(float& v, int, float x) { v = x; }

// dz and dx carry no __restrict__: dx may alias dz (every element is read, then written, by the one thread that owns it).
// part == nullptr (one workgroup of rows): dshift / dlog_scale are written here; otherwise part[blockIdx.y][2][per_sample] float64.
template <int V>
__global__ __launch_bounds__(ANB_COLS * ANB_SLICES) void actnorm_bwd_kernel(const float* dz, const float* __restrict__ z,
                                                                          const float* __restrict__ log_scale, long B, long per_sample,
                                                                          float* dx, float* __restrict__ dshift, float* __restrict__ dlog_scale,
                                                                          double* __restrict__ part) {
    typedef typename anb_vec<V>::type vec_t;
    __shared__ double red[2][ANB_SLICES][ANB_COLS * V];
    const bool sums = dshift || dlog_scale;
    const long i0 = ((long)blockIdx.x * ANB_COLS + threadIdx.x) * V;          // first column of this thread
    const bool live = i0 < per_sample;                                         // (per_sample % V == 0: all V columns or none)
    const long r0 = (long)blockIdx.y * ANB_ROWS;
    const long r1 = r0 + ANB_ROWS < B ? r0 + ANB_ROWS : B;
    const long len = (r1 - r0 + ANB_SLICES - 1) / ANB_SLICES;                  // rows per run
    const long b0 = r0 + threadIdx.y * len;
    const long b1 = b0 + len < r1 ? b0 + len : r1;
    double s_dx[V], s_dl[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s_dx[k] = s_dl[k] = 0.0;
    if (live) {
        float es[V];
        const vec_t ls = *reinterpret_cast<const vec_t*>(log_scale + i0);
#pragma unroll
        for (int k = 0; k < V; ++k) es[k] = expf(-anb_get<V>(ls, k));
        for (long b = b0; b < b1; ++b) {
            const long o = b * per_sample + i0;
            const vec_t g = *reinterpret_cast<const vec_t*>(dz + o);
            vec_t d;
#pragma unroll
            for (int k = 0; k < V; ++k) anb_set<V>(d, k, anb_get<V>(g, k) * es[k]);
            *reinterpret_cast<vec_t*>(dx + o) = d;
            if (dshift) {
#pragma unroll
                for (int k = 0; k < V; ++k) s_dx[k] += (double)anb_get<V>(d, k);
            }
            if (dlog_scale) {
                const vec_t y = *reinterpret_cast<const vec_t*>(z + o);
#pragma unroll
                for (int k = 0; k < V; ++k) s_dl[k] += (double)anb_get<V>(g, k) * (double)anb_get<V>(y, k);
            }
        }
    }
    if (!sums) return;                                                         // (uniform over the grid: no barrier is skipped by a part of a workgroup)
#pragma unroll
    for (int k = 0; k < V; ++k) {
        red[0][threadIdx.y][threadIdx.x * V + k] = s_dx[k];
        red[1][threadIdx.y][threadIdx.x * V + k] = s_dl[k];
    }
    __syncthreads();
    if (threadIdx.y != 0 || !live) return;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        double a = 0.0, c = 0.0;
        for (int s = 0; s < ANB_SLICES; ++s) {                                 // the runs in index order
            a += red[0][s][threadIdx.x * V + k];
            c += red[1][s][threadIdx.x * V + k];
        }
        if (part) {
            double* p = part + (long)blockIdx.y * 2 * per_sample;
            p[i0 + k] = a;
            p[per_sample + i0 + k] = c;
        } else {
            if (dshift) dshift[i0 + k] = (float)(-a);
            if (dlog_scale) dlog_scale[i0 + k] = (float)(-c);
        }
    }
}

// second stage: the workgroups' partials in index order, one rounding
__global__ __launch_bounds__(256) void actnorm_bwd_combine_kernel(const double* __restrict__ part, long per_sample, int chunks,
                                                                  float* __restrict__ dshift, float* __restrict__ dlog_scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_sample) return;
    double a = 0.0, c = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const double* p = part + (long)k * 2 * per_sample;
        a += p[i];
        c += p[per_sample + i];
    }
    if (dshift) dshift[i] = (float)(-a);
    if (dlog_scale) dlog_scale[i] = (float)(-c);
}

extern "C" int ldt_actnorm_bwd(const float* dz, const float* z, const float* log_scale, int64_t B, int64_t per_sample, float* dx, float* dshift,
                               float* dlog_scale, void* stream) {
    LDT_REQUIRE(dz && log_scale && dx && (z || !dlog_scale), LDT_EARG, "actnorm_bwd: null pointer (dlog_scale needs z)");
    LDT_REQUIRE(B >= 1 && per_sample >= 1, LDT_EARG, "actnorm_bwd: B %ld, per_sample %ld", (long)B, (long)per_sample);
    hipStream_t s = ldt_stream(stream);
    const bool sums = dshift || dlog_scale;
    const bool vec = per_sample % 4 == 0 && ldt_aligned16(dz) && ldt_aligned16(dx) && ldt_aligned16(log_scale) && (!dlog_scale || ldt_aligned16(z));
    const int V = vec ? 4 : 1;
    const long groups = (per_sample / V + ANB_COLS - 1) / ANB_COLS;
    const long chunks = (B + ANB_ROWS - 1) / ANB_ROWS;
    LDT_REQUIRE(groups <= 0x7fffffffL && chunks <= 65535 && (per_sample + 255) / 256 <= 0x7fffffffL, LDT_ESHAPE,
                "actnorm_bwd: B %ld, per_sample %ld", B, per_sample);
    double* part = nullptr;
    if (sums && chunks > 1) {                                                  // stream-ordered scratch for the partials, released behind the second stage
        const hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&part), (size_t)chunks * 2 * (size_t)per_sample * sizeof(double), s);
        if (e != hipSuccess) { ldt_set_error("actnorm_bwd: hipMallocAsync: %s", hipGetErrorString(e)); return (int)e; }
    }
    const dim3 grid((unsigned)groups, (unsigned)chunks), block(ANB_COLS, ANB_SLICES);
    if (vec) hipLaunchKernelGGL(actnorm_bwd_kernel<4>, grid, block, 0, s, dz, z, log_scale, B, per_sample, dx, dshift, dlog_scale, part);
    else hipLaunchKernelGGL(actnorm_bwd_kernel<1>, grid, block, 0, s, dz, z, log_scale, B, per_sample, dx, dshift, dlog_scale, part);
    int rc = ldt_check_launch("actnorm_bwd");
    if (part) {
        if (rc == LDT_OK) {
            hipLaunchKernelGGL(actnorm_bwd_combine_kernel, dim3((unsigned)((per_sample + 255) / 256)), dim3(256), 0, s, part, per_sample, (int)chunks,
                               dshift, dlog_scale);
            rc = ldt_check_launch("actnorm_bwd (second stage)");
        }
        const hipError_t e = hipFreeAsync(part, s);
        if (e != hipSuccess && rc == LDT_OK) { ldt_set_error("actnorm_bwd: hipFreeAsync: %s", hipGetErrorString(e)); rc = (int)e; }
    }
    return rc;
}
