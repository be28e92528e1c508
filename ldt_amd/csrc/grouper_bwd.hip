// Backward of the LocalGrouper's data movement (gfx950): what lies around the three PreExtraction GEMMs when the Compressor's front is trained
// (model/Compressor/layers.py:288-319 LocalGrouper.forward with normalize = 'anchor', :186 the max over the k neighbours; Network.py:97
// MiniPointnet's max over the tokens).
//     ldt_maxpool_argmax        ldt_maxpool's values (bit for bit) with the arg-max row of every (group, channel); on equal values the
//                               smallest index wins, as torch.max on the CPU; optionally ReLU on the maximum (max_j ReLU(z_j) = ReLU(max_j z_j))
//     ldt_maxpool_relu_bwd      out = max_j ReLU(z_j): d_out goes to the kept row, and only where out > 0; every other element is written 0
//     ldt_group_normalize_bwd   U = [alpha (g - anchor) / (std + 1e-5) + beta | anchor features]: dalpha, dbeta and the gradient of the
//                               point features, the statistics term included
// The training kernels' contract (actnorm.hip, score_bwd.hip): no floating-point atomics, every sum in a fixed order with float64 partials
// and one rounding, two runs of one input give the same bits.  The scatter dfeat[b, knn[s, j]] += ... is a GATHER here: the caller hands
// over the inverted index of knn_idx (per point its (s, j) entries in ascending order) and one workgroup per destination point adds its
// entries in that order, then the groups it is the centre of in ascending s.  The per-sample statistics are the forward's own
// (ldt_group_stats_launch, order-independent fixed-point sums), so the backward differentiates the inv the forward multiplied with.
#include "../../include/ldt_hip.h"
#include "kernels.h"

// ---------------------------------------------------------------- the max over the middle axis with its arg-max, and its backward
// A NaN in a column is the result, as in ldt_maxpool; the FIRST NaN is kept (torch.max).
template <typename TI>
__global__ __launch_bounds__(256) void maxpool_argmax_kernel(const TI* __restrict__ in, long ld, int n, int C, float* __restrict__ out,
                                                             int* __restrict__ arg, long G, int relu) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < G * C; i += (long)gridDim.x * 256L) {
        const long g = i / C; const int c = (int)(i % C);
        float m = -INFINITY;
        int a = 0;
        for (int j = 0; j < n; ++j) {
            const float v = (float)in[(g * n + j) * ld + c];
            if (v > m || (v != v && m == m)) { m = v; a = j; }
        }
        out[i] = (relu && m <= 0.f) ? 0.f : m;                            // (a NaN stays a NaN)
        arg[i] = a;
    }
}

extern "C" int ldt_maxpool_argmax(const void* in, int32_t in_bf16, int64_t ld, int64_t G, int32_t n, int32_t C, float* out, int32_t* arg, int32_t relu,
                                  void* stream) {
    LDT_REQUIRE(in && out && arg, LDT_EARG, "maxpool_argmax: null pointer");
    LDT_REQUIRE(G > 0 && n > 0 && C > 0 && ld >= C, LDT_ESHAPE, "maxpool_argmax: bad shape");
    const dim3 grid(ldt_grid_1d(G * C, 256, 4096)), block(256);
    if (in_bf16) hipLaunchKernelGGL(maxpool_argmax_kernel<bf16_t>, grid, block, 0, ldt_stream(stream), ldt_bf16(in), (long)ld, n, C, out, arg, (long)G, (int)relu);
    else hipLaunchKernelGGL(maxpool_argmax_kernel<float>, grid, block, 0, ldt_stream(stream), (const float*)in, (long)ld, n, C, out, arg, (long)G, (int)relu);
    return ldt_check_launch("maxpool_argmax");
}

// dz[g][j][c] = d_out[g][c] where j == arg[g][c] and out[g][c] > 0, else 0: every element of dz is written, a thread owns V columns of a row
template <int V>
__global__ __launch_bounds__(256) void maxpool_relu_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ out,
                                                               const int* __restrict__ arg, long G, int n, int C, float* __restrict__ dz, long ld) {
    const long per = C / V, total = G * n * per;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long row = i / per;
        const int c0 = (int)(i - row * per) * V;
        const long g = row / n;
        const int j = (int)(row - g * n);
        if (V == 4) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(d_out + g * C + c0), o = *reinterpret_cast<const f32x4*>(out + g * C + c0);
            const int4 a = *reinterpret_cast<const int4*>(arg + g * C + c0);
            f32x4 r;
            r[0] = (a.x == j && o[0] > 0.f) ? d[0] : 0.f;
            r[1] = (a.y == j && o[1] > 0.f) ? d[1] : 0.f;
            r[2] = (a.z == j && o[2] > 0.f) ? d[2] : 0.f;
            r[3] = (a.w == j && o[3] > 0.f) ? d[3] : 0.f;
            *reinterpret_cast<f32x4*>(dz + row * ld + c0) = r;
        } else {
            dz[row * ld + c0] = (arg[g * C + c0] == j && out[g * C + c0] > 0.f) ? d_out[g * C + c0] : 0.f;
        }
    }
}

extern "C" int ldt_maxpool_relu_bwd(const float* d_out, const float* out, const int32_t* arg, int64_t G, int32_t n, int32_t C, float* dz, int64_t ld,
                                    void* stream) {
    LDT_REQUIRE(d_out && out && arg && dz, LDT_EARG, "maxpool_relu_bwd: null pointer");
    LDT_REQUIRE(G > 0 && n > 0 && C > 0 && ld >= C, LDT_ESHAPE, "maxpool_relu_bwd: bad shape");
    const bool vec = C % 4 == 0 && ld % 4 == 0 && ldt_aligned16(d_out) && ldt_aligned16(out) && ldt_aligned16(arg) && ldt_aligned16(dz);
    const long items = G * n * (long)(C / (vec ? 4 : 1));
    const dim3 grid(ldt_grid_1d(items, 256, 8192)), block(256);
    if (vec) hipLaunchKernelGGL(maxpool_relu_bwd_kernel<4>, grid, block, 0, ldt_stream(stream), d_out, out, arg, (long)G, n, C, dz, (long)ld);
    else hipLaunchKernelGGL(maxpool_relu_bwd_kernel<1>, grid, block, 0, ldt_stream(stream), d_out, out, arg, (long)G, n, C, dz, (long)ld);
    return ldt_check_launch("maxpool_relu_bwd");
}

// ---------------------------------------------------------------- the 'anchor' normalisation's backward
#define GNB_COLS 64                  // columns per workgroup of the column sums (one wave reads 256 contiguous bytes of a row)
#define GNB_SLICES 4                 // row runs per workgroup
#define GNB_ROWS 256                 // grouped rows per workgroup

// The forward's per-sample numbers (pointops.hip, group_build_kernel), from the same sums in the same operations
struct GnbSample { double mean; float sigma; float inv; };
__device__ __forceinline__ GnbSample gnb_sample(const double* __restrict__ stats, int b, double cnt) {
    GnbSample r;
    r.mean = fx_load(&stats[2 * b]) / cnt;
    const double var = (fx_load(&stats[2 * b + 1]) - cnt * r.mean * r.mean) / (cnt - 1.0);
    r.sigma = (float)sqrt(var > 0.0 ? var : 0.0);
    r.inv = 1.0f / (r.sigma + 1e-5f);
    return r;
}
// d = g - anchor as the forward rounds it (fp32), for column c < D + 3 of grouped row (point pi, centre ci) of sample b
__device__ __forceinline__ float gnb_d(const float* __restrict__ feat, const float* __restrict__ xyz, long b, int n, int D, int pi, int ci, int c) {
    return c < D ? feat[(b * n + pi) * D + c] - feat[(b * n + ci) * D + c] : xyz[(b * n + pi) * 3 + (c - D)] - xyz[(b * n + ci) * 3 + (c - D)];
}

// part[b][chunk][0][c] = sum over the chunk's rows of dU[., c], [1][c] = of dU[., c] * d[., c] (exact float64 products), c < D + 3
template <typename TI>
__global__ __launch_bounds__(GNB_COLS * GNB_SLICES) void gnb_colsum_kernel(const TI* __restrict__ dU, long ld, const float* __restrict__ feat,
                                                                           const float* __restrict__ xyz, const int* __restrict__ fps_idx,
                                                                           const int* __restrict__ knn_idx, int n, int S, int k, int D,
                                                                           double* __restrict__ part) {
    __shared__ double red[2][GNB_SLICES][GNB_COLS];
    const int D3 = D + 3, b = blockIdx.z;
    const int c = blockIdx.x * GNB_COLS + threadIdx.x;
    const long rows = (long)S * k;
    const long r0 = (long)blockIdx.y * GNB_ROWS;
    const long r1 = r0 + GNB_ROWS < rows ? r0 + GNB_ROWS : rows;
    const long len = (r1 - r0 + GNB_SLICES - 1) / GNB_SLICES;
    const long a0 = r0 + threadIdx.y * len;
    const long a1 = a0 + len < r1 ? a0 + len : r1;
    double s0 = 0.0, s1 = 0.0;
    if (c < D3) {
        for (long r = a0; r < a1; ++r) {
            const int ci = fps_idx[(long)b * S + r / k], pi = knn_idx[(long)b * rows + r];
            if ((unsigned)ci >= (unsigned)n || (unsigned)pi >= (unsigned)n) continue;      // (an index outside the cloud contributes nothing)
            const float u = (float)dU[((long)b * rows + r) * ld + c];
            s0 += (double)u;
            s1 += (double)u * (double)gnb_d(feat, xyz, b, n, D, pi, ci, c);
        }
    }
    red[0][threadIdx.y][threadIdx.x] = s0;
    red[1][threadIdx.y][threadIdx.x] = s1;
    __syncthreads();
    if (threadIdx.y != 0 || c >= D3) return;
    double a = 0.0, e = 0.0;
    for (int s = 0; s < GNB_SLICES; ++s) { a += red[0][s][threadIdx.x]; e += red[1][s][threadIdx.x]; }
    double* p = part + ((long)b * gridDim.y + blockIdx.y) * 2 * D3;
    p[c] = a;
    p[D3 + c] = e;
}

// sab[b][0 | 1][c] = the chunks of sample b in index order
__global__ __launch_bounds__(256) void gnb_combine_kernel(const double* __restrict__ part, int chunks, int D3, double* __restrict__ sab) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= D3) return;
    double a = 0.0, e = 0.0;
    for (int q = 0; q < chunks; ++q) {
        const double* p = part + ((long)b * chunks + q) * 2 * D3;
        a += p[c];
        e += p[D3 + c];
    }
    sab[(long)b * 2 * D3 + c] = a;
    sab[(long)b * 2 * D3 + D3 + c] = e;
}

// One workgroup.  Per sample: coef[b] = (inv, P inv^2 / ((n_el - 1) sigma), mean) with P = sum_c alpha[c] sab[b][1][c] in column order (the
// second entry 0 where sigma == 0: the statistics term is dropped, see include/ldt_hip.h).  Per column: dbeta = sum_b sab[b][0][c],
// dalpha = sum_b inv_b sab[b][1][c] in sample order, one rounding each.
__global__ __launch_bounds__(256) void gnb_finish_kernel(const double* __restrict__ sab, const double* __restrict__ stats, const float* __restrict__ alpha,
                                                         int B, int D3, double cnt, double* __restrict__ coef, float* __restrict__ dalpha,
                                                         float* __restrict__ dbeta) {
    for (int b = threadIdx.x; b < B; b += 256) {
        const GnbSample sm = gnb_sample(stats, b, cnt);
        double P = 0.0;
        for (int c = 0; c < D3; ++c) P += (double)alpha[c] * sab[(long)b * 2 * D3 + D3 + c];
        const double inv = (double)sm.inv;
        coef[3 * b] = inv;
        coef[3 * b + 1] = sm.sigma > 0.f ? P * inv * inv / ((cnt - 1.0) * (double)sm.sigma) : 0.0;
        coef[3 * b + 2] = sm.mean;
    }
    for (int c = threadIdx.x; c < D3; c += 256) {
        double a = 0.0, e = 0.0;
        for (int b = 0; b < B; ++b) {
            a += sab[(long)b * 2 * D3 + c];
            e += (double)gnb_sample(stats, b, cnt).inv * sab[(long)b * 2 * D3 + D3 + c];
        }
        if (dbeta) dbeta[c] = (float)a;
        if (dalpha) dalpha[c] = (float)e;
    }
}

// dd of grouped row `e` (point pi, centre ci), column c < D, in float64 from the fp32 d the forward formed
template <typename TI>
__device__ __forceinline__ double gnb_dd(const TI* __restrict__ dU, long ld, const float* __restrict__ feat, long b, int n, int D, long rows, long e,
                                         int pi, int ci, int c, double alpha_c, const double* __restrict__ cf) {
    const double u = (double)(float)dU[(b * rows + e) * ld + c];
    const double d = (double)(feat[(b * n + pi) * D + c] - feat[(b * n + ci) * D + c]);
    return alpha_c * u * cf[0] - cf[1] * (d - cf[2]);
}

// anch[b][s][c] = -sum_j dd[s, j, c] + sum_j dU[s, j, D + 3 + c] in the order of j (float64): what group s hands to its centre point
template <typename TI>
__global__ __launch_bounds__(128) void gnb_anchor_kernel(const TI* __restrict__ dU, long ld, const float* __restrict__ feat, const int* __restrict__ fps_idx,
                                                         const int* __restrict__ knn_idx, const float* __restrict__ alpha, const double* __restrict__ coef,
                                                         int n, int S, int k, int D, double* __restrict__ anch) {
    const int s = blockIdx.x, b = blockIdx.y;
    const long rows = (long)S * k;
    const int ci = fps_idx[(long)b * S + s];
    const double cf[3] = {coef[3 * b], coef[3 * b + 1], coef[3 * b + 2]};
    for (int c = threadIdx.x; c < D; c += 128) {
        double acc = 0.0;
        if ((unsigned)ci < (unsigned)n) {
            const double al = (double)alpha[c];
            for (int j = 0; j < k; ++j) {
                const long e = (long)s * k + j;
                const int pi = knn_idx[(long)b * rows + e];
                if ((unsigned)pi >= (unsigned)n) continue;
                acc -= gnb_dd(dU, ld, feat, (long)b, n, D, rows, e, pi, ci, c, al, cf);
                acc += (double)(float)dU[((long)b * rows + e) * ld + D + 3 + c];
            }
        }
        anch[((long)b * S + s) * D + c] = acc;
    }
}

// dfeat[b][p][c] = sum over the entries e of point p (ascending) of dd[e][c], then over the groups s with fps[s] == p (ascending) of
// anch[b][s][c]: float64, one rounding.  A point in no group and centre of none gets exactly 0.
template <typename TI>
__global__ __launch_bounds__(128) void gnb_gather_kernel(const TI* __restrict__ dU, long ld, const float* __restrict__ feat, const int* __restrict__ fps_idx,
                                                         const int* __restrict__ inv_start, const int* __restrict__ inv_entry,
                                                         const float* __restrict__ alpha, const double* __restrict__ coef,
                                                         const double* __restrict__ anch, int n, int S, int k, int D, float* __restrict__ dfeat) {
    const int p = blockIdx.x, b = blockIdx.y;
    const long rows = (long)S * k;
    const double cf[3] = {coef[3 * b], coef[3 * b + 1], coef[3 * b + 2]};
    int e0 = inv_start[(long)b * (n + 1) + p], e1 = inv_start[(long)b * (n + 1) + p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > rows) e1 = (int)rows;
    for (int c = threadIdx.x; c < D; c += 128) {
        const double al = (double)alpha[c];
        double acc = 0.0;
        for (int q = e0; q < e1; ++q) {
            const int e = inv_entry[(long)b * rows + q];
            if ((unsigned)e >= (unsigned)rows) continue;
            const int ci = fps_idx[(long)b * S + e / k];
            if ((unsigned)ci >= (unsigned)n) continue;
            acc += gnb_dd(dU, ld, feat, (long)b, n, D, rows, (long)e, p, ci, c, al, cf);
        }
        for (int s = 0; s < S; ++s)
            if (fps_idx[(long)b * S + s] == p) acc += anch[((long)b * S + s) * D + c];
        dfeat[((long)b * n + p) * D + c] = (float)acc;
    }
}

template <typename TI>
static int gnb_run(const TI* dU, long ld, const float* feat, const float* xyz, const int* fps_idx, const int* knn_idx, const int* inv_start,
                   const int* inv_entry, const float* alpha, int B, int n, int S, int k, int D, float* dalpha, float* dbeta, float* dfeat, hipStream_t s) {
    const int D3 = D + 3;
    const long rows = (long)S * k;
    const long chunks = (rows + GNB_ROWS - 1) / GNB_ROWS;
    const size_t n_part = (size_t)B * chunks * 2 * D3, n_sab = (size_t)B * 2 * D3, n_coef = 3 * (size_t)B, n_anch = (size_t)B * S * D, n_stats = 2 * (size_t)B;
    double* ws = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&ws), (n_part + n_sab + n_coef + n_anch + n_stats) * sizeof(double), s);
    if (e != hipSuccess) { ldt_set_error("group_normalize_bwd: hipMallocAsync: %s", hipGetErrorString(e)); return (int)e; }
    double *part = ws, *sab = part + n_part, *coef = sab + n_sab, *anch = coef + n_coef, *stats = anch + n_anch;
    int rc = ldt_group_stats_launch(feat, xyz, fps_idx, knn_idx, stats, B, n, S, k, D, s);
    if (rc == LDT_OK) {
        hipLaunchKernelGGL(gnb_colsum_kernel<TI>, dim3((unsigned)((D3 + GNB_COLS - 1) / GNB_COLS), (unsigned)chunks, (unsigned)B), dim3(GNB_COLS, GNB_SLICES), 0, s,
                           dU, ld, feat, xyz, fps_idx, knn_idx, n, S, k, D, part);
        rc = ldt_check_launch("group_normalize_bwd (sums)");
    }
    if (rc == LDT_OK) {
        hipLaunchKernelGGL(gnb_combine_kernel, dim3((unsigned)((D3 + 255) / 256), (unsigned)B), dim3(256), 0, s, part, (int)chunks, D3, sab);
        rc = ldt_check_launch("group_normalize_bwd (second stage)");
    }
    if (rc == LDT_OK) {
        hipLaunchKernelGGL(gnb_finish_kernel, dim3(1), dim3(256), 0, s, sab, stats, alpha, B, D3, (double)rows * D3, coef, dalpha, dbeta);
        rc = ldt_check_launch("group_normalize_bwd (coefficients)");
    }
    if (rc == LDT_OK && dfeat) {
        hipLaunchKernelGGL(gnb_anchor_kernel<TI>, dim3((unsigned)S, (unsigned)B), dim3(128), 0, s, dU, ld, feat, fps_idx, knn_idx, alpha, coef, n, S, k, D, anch);
        rc = ldt_check_launch("group_normalize_bwd (centres)");
    }
    if (rc == LDT_OK && dfeat) {
        hipLaunchKernelGGL(gnb_gather_kernel<TI>, dim3((unsigned)n, (unsigned)B), dim3(128), 0, s, dU, ld, feat, fps_idx, inv_start, inv_entry, alpha, coef, anch,
                           n, S, k, D, dfeat);
        rc = ldt_check_launch("group_normalize_bwd (points)");
    }
    e = hipFreeAsync(ws, s);
    if (e != hipSuccess && rc == LDT_OK) { ldt_set_error("group_normalize_bwd: hipFreeAsync: %s", hipGetErrorString(e)); rc = (int)e; }
    return rc;
}

extern "C" int ldt_group_normalize_bwd(const void* dU, int32_t dU_bf16, int64_t ld, const float* feat, const float* xyz, const int32_t* fps_idx,
                                       const int32_t* knn_idx, const int32_t* inv_start, const int32_t* inv_entry, const float* alpha, int32_t B,
                                       int32_t n, int32_t S, int32_t k, int32_t D, float* dalpha, float* dbeta, float* dfeat, void* stream) {
    LDT_REQUIRE(dU && feat && xyz && fps_idx && knn_idx && alpha, LDT_EARG, "group_normalize_bwd: null pointer");
    LDT_REQUIRE(!dfeat || (inv_start && inv_entry), LDT_EARG, "group_normalize_bwd: dfeat needs the inverted index of knn_idx");
    LDT_REQUIRE(B > 0 && n > 0 && S > 0 && k > 0 && D > 0 && ld >= 2 * (int64_t)D + 3, LDT_ESHAPE, "group_normalize_bwd: bad shape");
    LDT_REQUIRE((int64_t)S * k * (D + 3) >= 2, LDT_ESHAPE, "group_normalize_bwd: the unbiased std needs at least two grouped elements per sample");
    LDT_REQUIRE((int64_t)S * k <= 0x7fffffffLL && B <= 65535 && ((int64_t)S * k + GNB_ROWS - 1) / GNB_ROWS <= 65535, LDT_ESHAPE,
                "group_normalize_bwd: B %d, S %d, k %d", (int)B, (int)S, (int)k);
    hipStream_t s = ldt_stream(stream);
    if (dU_bf16) return gnb_run<bf16_t>(ldt_bf16(dU), (long)ld, feat, xyz, fps_idx, knn_idx, inv_start, inv_entry, alpha, B, n, S, k, D, dalpha, dbeta, dfeat, s);
    return gnb_run<float>((const float*)dU, (long)ld, feat, xyz, fps_idx, knn_idx, inv_start, inv_entry, alpha, B, n, S, k, D, dalpha, dbeta, dfeat, s);
}
