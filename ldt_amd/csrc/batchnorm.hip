// Training-mode BatchNorm1d + ReLU over the rows of a [M][C] activation (gfx950): the front of the Compressor (model/Compressor/layers.py:
// 115-160 PreExtraction, Network.py:86-101 MiniPointnet) normalises with BATCH statistics while it is trained.
//     ldt_bn_stats      mean[c], rstd[c] = 1 / sqrt(biased var + eps) over the M rows; optionally the running buffers as nn.BatchNorm1d
//                       updates them (momentum, UNBIASED variance into running_var)
//     ldt_bn_relu_fwd   y = ReLU(gamma * xhat + beta), xhat = (x - mean) * rstd, to bf16 or fp32
//     ldt_bn_relu_bwd   dyh = dy [y > 0];  dgamma = sum dyh xhat, dbeta = sum dyh;  dx = gamma rstd (dyh - dbeta / M - xhat dgamma / M)
// xhat and the mask are never stored: the backward recomputes them from the saved x with bn_xhat / bn_pre, the forward's own two lines.
// What these kernels share with actnorm.hip and score_bwd.hip:
//   * no atomics, a fixed order: a workgroup owns BN_ROWS rows of BN_COLS * V columns, cut into BN_SLICES contiguous runs, each summed in
//     row order and the runs added in index order; every workgroup writes its float64 partial and a second kernel adds the partials in index
//     order.  Two runs of one input give the same bits;
//   * the sums are carried in float64 and rounded to fp32 once.  The mean is formed first and the variance is the mean of (x - mean)^2 with
//     the float64 mean (two passes over x): a column of equal values has variance exactly 0, rstd = 1 / sqrt(eps);
//   * a thread owns V columns (V = 4: 16-byte loads; V = 1: the scalar form of the same kernel, any width, stride or alignment).
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define BN_COLS 16                  // column groups (of V columns) per workgroup
#define BN_SLICES 16                 // row runs per workgroup
#define BN_ROWS 512                  // rows per workgroup

template <int V> struct bn_vec;
template <> struct bn_vec<4> { typedef f32x4 type; typedef bf16x4 btype; };
template <> struct bn_vec<1> { typedef float type; typedef bf16_t btype; };
template <int V> __device__ __forceinline__ float bn_get(const typename bn_vec<V>::type& v, int k);
template <> __device__ __forceinline__ float bn_get<4>(const f32x4& v, int k) { return v[k]; }
template <> __device__ __forceinline__ float bn_get<1>(const float& v, int) { return v; }
template <int V> __device__ __forceinline__ void bn_set(typename bn_vec<V>::type& v, int k, float x);
template <> __device__ __forceinline__ void bn_set<4>(f32x4& v, int k, float x) { v[k] = x; }
template <> __device__ __forceinline__ void bn_set<1>(float& v, int, float x) { v = x; }
template <int V> __device__ __forceinline__ void bn_setb(typename bn_vec<V>::btype& v, int k, float x);
template <> __device__ __forceinline__ void bn_setb<4>(bf16x4& v, int k, float x) { v[k] = (bf16_t)x; }
template <> __device__ __forceinline__ void bn_setb<1>(bf16_t& v, int, float x) { v = (bf16_t)x; }

// THE two lines of the normalisation: the forward and both passes of the backward form xhat and the pre-activation with them
__device__ __forceinline__ float bn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float bn_pre(float xh, float gamma, float beta) { return fmaf(gamma, xh, beta); }

// Column sums of a workgroup's rows -> part[blockIdx.y][2][C] float64.
//   MODE 0: sum x                            (second slot 0)
//   MODE 1: sum (x - mean64)^2, in float64   (second slot 0)
//   MODE 2: sum dyh, sum dyh * xhat          (dyh = dy where gamma * xhat + beta > 0, else 0; the products exact in float64)
template <int V, int MODE>
__global__ __launch_bounds__(BN_COLS * BN_SLICES) void bn_colsum_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ dy, long lddy,
                                                                        long M, int C, const double* __restrict__ mean64,
                                                                        const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, double* __restrict__ part) {
    typedef typename bn_vec<V>::type vec_t;
    __shared__ double red[2][BN_SLICES][BN_COLS * V];
    const long c0 = ((long)blockIdx.x * BN_COLS + threadIdx.x) * V;            // first column of this thread
    const bool live = c0 < C;                                                   // (V = 4 only with C % 4 == 0: all V columns or none)
    const long r0 = (long)blockIdx.y * BN_ROWS;
    const long r1 = r0 + BN_ROWS < M ? r0 + BN_ROWS : M;
    const long len = (r1 - r0 + BN_SLICES - 1) / BN_SLICES;                    // rows per run
    const long b0 = r0 + threadIdx.y * len;
    const long b1 = b0 + len < r1 ? b0 + len : r1;
    double s0[V], s1[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0.0;
    if (live) {
        double mu64[V];
        float mu[V], rs[V], ga[V], be[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            mu64[k] = MODE == 1 ? mean64[c0 + k] : 0.0;
            mu[k] = MODE == 2 ? stats[c0 + k] : 0.f;
            rs[k] = MODE == 2 ? stats[C + c0 + k] : 0.f;
            ga[k] = MODE == 2 ? gamma[c0 + k] : 0.f;
            be[k] = MODE == 2 ? beta[c0 + k] : 0.f;
        }
        for (long r = b0; r < b1; ++r) {
            const vec_t xv = *reinterpret_cast<const vec_t*>(x + r * ldx + c0);
            if (MODE == 0) {
#pragma unroll
                for (int k = 0; k < V; ++k) s0[k] += (double)bn_get<V>(xv, k);
            } else if (MODE == 1) {
#pragma unroll
                for (int k = 0; k < V; ++k) { const double d = (double)bn_get<V>(xv, k) - mu64[k]; s0[k] += d * d; }
            } else {
                const vec_t gv = *reinterpret_cast<const vec_t*>(dy + r * lddy + c0);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float xh = bn_xhat(bn_get<V>(xv, k), mu[k], rs[k]);
                    const float g = bn_pre(xh, ga[k], be[k]) > 0.f ? bn_get<V>(gv, k) : 0.f;
                    s0[k] += (double)g;
                    s1[k] += (double)g * (double)xh;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        red[0][threadIdx.y][threadIdx.x * V + k] = s0[k];
        red[1][threadIdx.y][threadIdx.x * V + k] = s1[k];
    }
    __syncthreads();
    if (threadIdx.y != 0 || !live) return;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        double a = 0.0, c = 0.0;
        for (int s = 0; s < BN_SLICES; ++s) {                                  // the runs in index order
            a += red[0][s][threadIdx.x * V + k];
            c += red[1][s][threadIdx.x * V + k];
        }
        double* p = part + (long)blockIdx.y * 2 * C;
        p[c0 + k] = a;
        p[C + c0 + k] = c;
    }
}

// The workgroups' partials part[k * stride + at], k = 0 .. chunks - 1, added in index order.  The loads go out BN_BATCH at a time: they do not
// depend on the running sum, and issued one behind the other each costs a memory latency (128 chunks at the shipped 65 536 rows: 31 us a
// second stage, three times the first stage's pass over x).
#define BN_BATCH 16
__device__ __forceinline__ double bn_sum_partials(const double* __restrict__ part, long stride, long at, int chunks) {
    double a = 0.0;
    for (int k0 = 0; k0 < chunks; k0 += BN_BATCH) {
        double v[BN_BATCH];
#pragma unroll
        for (int j = 0; j < BN_BATCH; ++j) v[j] = k0 + j < chunks ? part[(long)(k0 + j) * stride + at] : 0.0;
#pragma unroll
        for (int j = 0; j < BN_BATCH; ++j)
            if (k0 + j < chunks) a += v[j];
    }
    return a;
}

// second stage of MODE 0: mean64[c] = (the partials in index order) / M
__global__ __launch_bounds__(256) void bn_mean_kernel(const double* __restrict__ part, int C, int chunks, long M, double* __restrict__ mean64) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    mean64[c] = bn_sum_partials(part, 2L * C, c, chunks) / (double)M;
}

// second stage of MODE 1: the statistics, one rounding each, and the running buffers as nn.BatchNorm1d writes them in training mode
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ part, const double* __restrict__ mean64, int C, int chunks,
                                                              long M, double eps, float* __restrict__ stats, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var, double momentum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double a = bn_sum_partials(part, 2L * C, c, chunks);
    const double var = a / (double)M;
    stats[c] = (float)mean64[c];
    stats[C + c] = (float)(1.0 / sqrt(var + eps));
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean64[c]);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (a / (double)(M - 1)));
}

// second stage of MODE 2: dbeta, dgamma (one rounding each) and the two per-column means the row pass subtracts
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, int C, int chunks, long M, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double a = bn_sum_partials(part, 2L * C, c, chunks), g = bn_sum_partials(part, 2L * C, (long)C + c, chunks);
    if (dbeta) dbeta[c] = (float)a;
    if (dgamma) dgamma[c] = (float)g;
    coef[c] = (float)(a / (double)M);
    coef[C + c] = (float)(g / (double)M);
}

// y[r][c] = ReLU(gamma[c] * xhat + beta[c]) for c < C, 0 for C <= c < cols_pad (the K padding of a bf16 GEMM operand)
template <int V, bool OUT_BF16>
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const float* __restrict__ x, long ldx, long M, int C, int cols_pad,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, void* __restrict__ y, long ldy) {
    typedef typename bn_vec<V>::type vec_t;
    typedef typename bn_vec<V>::btype bvec_t;
    const long per = cols_pad / V, total = M * per;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / per;
        const int c0 = (int)(i - r * per) * V;
        vec_t o;
        if (c0 < C) {
            const vec_t xv = *reinterpret_cast<const vec_t*>(x + r * ldx + c0);
            const vec_t mu = *reinterpret_cast<const vec_t*>(stats + c0), rs = *reinterpret_cast<const vec_t*>(stats + C + c0);
            const vec_t ga = *reinterpret_cast<const vec_t*>(gamma + c0), be = *reinterpret_cast<const vec_t*>(beta + c0);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float p = bn_pre(bn_xhat(bn_get<V>(xv, k), bn_get<V>(mu, k), bn_get<V>(rs, k)), bn_get<V>(ga, k), bn_get<V>(be, k));
                bn_set<V>(o, k, p > 0.f ? p : (p != p ? p : 0.f));                            // (a NaN stays a NaN, as torch's relu)
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) bn_set<V>(o, k, 0.f);
        }
        if (OUT_BF16) {
            bvec_t ob;
#pragma unroll
            for (int k = 0; k < V; ++k) bn_setb<V>(ob, k, bn_get<V>(o, k));
            *reinterpret_cast<bvec_t*>(reinterpret_cast<bf16_t*>(y) + r * ldy + c0) = ob;
        } else {
            *reinterpret_cast<vec_t*>(reinterpret_cast<float*>(y) + r * ldy + c0) = o;
        }
    }
}

// dx[r][c] = (gamma rstd) * ((dyh - mean dyh) - xhat * mean(dyh xhat)); dy and dx carry no __restrict__: dx may alias dy (every element is
// read, then written, by the one thread that owns it)
template <int V>
__global__ __launch_bounds__(256) void bn_relu_bwd_rows_kernel(const float* dy, long lddy, const float* __restrict__ x, long ldx, long M, int C,
                                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ coef, float* dx, long lddx) {
    typedef typename bn_vec<V>::type vec_t;
    const long per = C / V, total = M * per;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long r = i / per;
        const int c0 = (int)(i - r * per) * V;
        const vec_t xv = *reinterpret_cast<const vec_t*>(x + r * ldx + c0);
        const vec_t gv = *reinterpret_cast<const vec_t*>(dy + r * lddy + c0);
        const vec_t mu = *reinterpret_cast<const vec_t*>(stats + c0), rs = *reinterpret_cast<const vec_t*>(stats + C + c0);
        const vec_t ga = *reinterpret_cast<const vec_t*>(gamma + c0), be = *reinterpret_cast<const vec_t*>(beta + c0);
        const vec_t mb = *reinterpret_cast<const vec_t*>(coef + c0), mg = *reinterpret_cast<const vec_t*>(coef + C + c0);
        vec_t o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xh = bn_xhat(bn_get<V>(xv, k), bn_get<V>(mu, k), bn_get<V>(rs, k));
            const float g = bn_pre(xh, bn_get<V>(ga, k), bn_get<V>(be, k)) > 0.f ? bn_get<V>(gv, k) : 0.f;
            const float t = fmaf(-xh, bn_get<V>(mg, k), g - bn_get<V>(mb, k));
            bn_set<V>(o, k, (bn_get<V>(ga, k) * bn_get<V>(rs, k)) * t);
        }
        *reinterpret_cast<vec_t*>(dx + r * lddx + c0) = o;
    }
}

// stream-ordered scratch of `n` doubles (released by bn_free behind the last kernel that reads it)
static int bn_alloc(double** p, size_t n, hipStream_t s, const char* who) {
    const hipError_t e = hipMallocAsync(reinterpret_cast<void**>(p), n * sizeof(double), s);
    if (e != hipSuccess) { ldt_set_error("%s: hipMallocAsync: %s", who, hipGetErrorString(e)); return (int)e; }
    return LDT_OK;
}
static int bn_free(double* p, hipStream_t s, int rc, const char* who) {
    const hipError_t e = hipFreeAsync(p, s);
    if (e != hipSuccess && rc == LDT_OK) { ldt_set_error("%s: hipFreeAsync: %s", who, hipGetErrorString(e)); return (int)e; }
    return rc;
}
// the grid of bn_colsum_kernel; false: a dimension does not fit
static bool bn_colsum_grid(long M, int C, int V, dim3* grid, long* chunks) {
    const long groups = ((long)C / V + BN_COLS - 1) / BN_COLS;
    *chunks = (M + BN_ROWS - 1) / BN_ROWS;
    if (groups > 0x7fffffffL || *chunks > 65535) return false;
    *grid = dim3((unsigned)groups, (unsigned)*chunks);
    return true;
}
#define BN_TRY(...)                          \
    do {                                     \
        if (rc == LDT_OK) { __VA_ARGS__; }   \
    } while (0)

extern "C" int ldt_bn_stats(const float* x, int64_t ldx, int64_t M, int32_t C, double eps, float* stats, float* running_mean, float* running_var,
                            double momentum, void* stream) {
    LDT_REQUIRE(x && stats, LDT_EARG, "bn_stats: null pointer");
    LDT_REQUIRE(M >= 2 && C >= 1 && ldx >= C, LDT_ESHAPE, "bn_stats: M %ld (training-mode BatchNorm needs more than one value per channel), C %d, ldx %ld",
                (long)M, (int)C, (long)ldx);
    LDT_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, LDT_EARG, "bn_stats: eps %g, momentum %g", eps, momentum);
    hipStream_t s = ldt_stream(stream);
    const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldt_aligned16(x);
    dim3 grid;
    long chunks;
    LDT_REQUIRE(bn_colsum_grid(M, C, vec ? 4 : 1, &grid, &chunks), LDT_ESHAPE, "bn_stats: M %ld, C %d", (long)M, (int)C);
    double* part = nullptr;
    int rc = bn_alloc(&part, (size_t)(chunks * 2 + 1) * (size_t)C, s, "bn_stats");
    if (rc != LDT_OK) return rc;
    double* mean64 = part + chunks * 2 * (long)C;
    const dim3 block(BN_COLS, BN_SLICES), fin((unsigned)((C + 255) / 256));
    if (vec) hipLaunchKernelGGL((bn_colsum_kernel<4, 0>), grid, block, 0, s, x, (long)ldx, nullptr, 0L, (long)M, (int)C, nullptr, nullptr, nullptr, nullptr, part);
    else hipLaunchKernelGGL((bn_colsum_kernel<1, 0>), grid, block, 0, s, x, (long)ldx, nullptr, 0L, (long)M, (int)C, nullptr, nullptr, nullptr, nullptr, part);
    rc = ldt_check_launch("bn_stats (sums)");
    BN_TRY(hipLaunchKernelGGL(bn_mean_kernel, fin, dim3(256), 0, s, part, (int)C, (int)chunks, (long)M, mean64); rc = ldt_check_launch("bn_stats (mean)"));
    BN_TRY(if (vec) hipLaunchKernelGGL((bn_colsum_kernel<4, 1>), grid, block, 0, s, x, (long)ldx, nullptr, 0L, (long)M, (int)C, mean64, nullptr, nullptr, nullptr, part);
           else hipLaunchKernelGGL((bn_colsum_kernel<1, 1>), grid, block, 0, s, x, (long)ldx, nullptr, 0L, (long)M, (int)C, mean64, nullptr, nullptr, nullptr, part);
           rc = ldt_check_launch("bn_stats (squares)"));
    BN_TRY(hipLaunchKernelGGL(bn_stats_finish_kernel, fin, dim3(256), 0, s, part, mean64, (int)C, (int)chunks, (long)M, eps, stats, running_mean,
                              running_var, momentum);
           rc = ldt_check_launch("bn_stats (second stage)"));
    return bn_free(part, s, rc, "bn_stats");
}

extern "C" int ldt_bn_relu_fwd(const float* x, int64_t ldx, int64_t M, int32_t C, const float* stats, const float* gamma, const float* beta, void* y,
                               int64_t ldy, int32_t out_bf16, int32_t cols_pad, void* stream) {
    LDT_REQUIRE(x && stats && gamma && beta && y, LDT_EARG, "bn_relu_fwd: null pointer");
    LDT_REQUIRE(M >= 1 && C >= 1 && ldx >= C && cols_pad >= C && ldy >= cols_pad, LDT_ESHAPE, "bn_relu_fwd: M %ld, C %d, ldx %ld, cols_pad %d, ldy %ld",
                (long)M, (int)C, (long)ldx, (int)cols_pad, (long)ldy);
    const bool vec = C % 4 == 0 && cols_pad % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldt_aligned16(x) && ldt_aligned16(stats) && ldt_aligned16(gamma) &&
                     ldt_aligned16(beta) && (out_bf16 ? (reinterpret_cast<uintptr_t>(y) & 7u) == 0 : ldt_aligned16(y));
    const long items = M * (long)(cols_pad / (vec ? 4 : 1));
    const dim3 grid(ldt_grid_1d(items, 256, 8192)), block(256);
    hipStream_t s = ldt_stream(stream);
    if (vec && out_bf16) hipLaunchKernelGGL((bn_relu_fwd_kernel<4, true>), grid, block, 0, s, x, (long)ldx, (long)M, (int)C, (int)cols_pad, stats, gamma, beta, y, (long)ldy);
    else if (vec) hipLaunchKernelGGL((bn_relu_fwd_kernel<4, false>), grid, block, 0, s, x, (long)ldx, (long)M, (int)C, (int)cols_pad, stats, gamma, beta, y, (long)ldy);
    else if (out_bf16) hipLaunchKernelGGL((bn_relu_fwd_kernel<1, true>), grid, block, 0, s, x, (long)ldx, (long)M, (int)C, (int)cols_pad, stats, gamma, beta, y, (long)ldy);
    else hipLaunchKernelGGL((bn_relu_fwd_kernel<1, false>), grid, block, 0, s, x, (long)ldx, (long)M, (int)C, (int)cols_pad, stats, gamma, beta, y, (long)ldy);
    return ldt_check_launch("bn_relu_fwd");
}

extern "C" int ldt_bn_relu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int32_t C, const float* stats, const float* gamma,
                               const float* beta, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* stream) {
    LDT_REQUIRE(dy && x && stats && gamma && beta && dx, LDT_EARG, "bn_relu_bwd: null pointer");
    LDT_REQUIRE(M >= 2 && C >= 1 && lddy >= C && ldx >= C && lddx >= C, LDT_ESHAPE, "bn_relu_bwd: M %ld, C %d, row strides %ld / %ld / %ld", (long)M, (int)C,
                (long)lddy, (long)ldx, (long)lddx);
    hipStream_t s = ldt_stream(stream);
    const bool vec = C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && ldt_aligned16(dy) && ldt_aligned16(x) && ldt_aligned16(dx) &&
                     ldt_aligned16(stats) && ldt_aligned16(gamma) && ldt_aligned16(beta);
    dim3 grid;
    long chunks;
    LDT_REQUIRE(bn_colsum_grid(M, C, vec ? 4 : 1, &grid, &chunks), LDT_ESHAPE, "bn_relu_bwd: M %ld, C %d", (long)M, (int)C);
    double* part = nullptr;
    int rc = bn_alloc(&part, (size_t)(chunks * 2 + 1) * (size_t)C, s, "bn_relu_bwd");              // (+ the two coefficient rows: 2 C floats, 16-byte aligned behind 16 chunks C bytes)
    if (rc != LDT_OK) return rc;
    float* coef = reinterpret_cast<float*>(part + chunks * 2 * (long)C);
    const dim3 block(BN_COLS, BN_SLICES), fin((unsigned)((C + 255) / 256));
    if (vec) hipLaunchKernelGGL((bn_colsum_kernel<4, 2>), grid, block, 0, s, x, (long)ldx, dy, (long)lddy, (long)M, (int)C, nullptr, stats, gamma, beta, part);
    else hipLaunchKernelGGL((bn_colsum_kernel<1, 2>), grid, block, 0, s, x, (long)ldx, dy, (long)lddy, (long)M, (int)C, nullptr, stats, gamma, beta, part);
    rc = ldt_check_launch("bn_relu_bwd (sums)");
    BN_TRY(hipLaunchKernelGGL(bn_bwd_finish_kernel, fin, dim3(256), 0, s, part, (int)C, (int)chunks, (long)M, dgamma, dbeta, coef);
           rc = ldt_check_launch("bn_relu_bwd (second stage)"));
    const long items = M * (long)(C / (vec ? 4 : 1));
    const dim3 rgrid(ldt_grid_1d(items, 256, 8192));
    BN_TRY(if (vec) hipLaunchKernelGGL(bn_relu_bwd_rows_kernel<4>, rgrid, dim3(256), 0, s, dy, (long)lddy, x, (long)ldx, (long)M, (int)C, stats, gamma, beta, coef, dx, (long)lddx);
           else hipLaunchKernelGGL(bn_relu_bwd_rows_kernel<1>, rgrid, dim3(256), 0, s, dy, (long)lddy, x, (long)ldx, (long)M, (int)C, stats, gamma, beta, coef, dx, (long)lddx);
           rc = ldt_check_launch("bn_relu_bwd (rows)"));
    return bn_free(part, s, rc, "bn_relu_bwd");
}
