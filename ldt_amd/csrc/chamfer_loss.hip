// The Chamfer reconstruction loss of Compressor training (evaluation/loss.py:71-78 CD_loss over chamfer3D.cu's forward / backward; gfx950):
// nearest neighbours with their indices, the loss on the device, and its gradient with respect to the estimated cloud.
//   ldt_chamfer_nn      d1[b][i] = min_j |x1_i - x2_j|^2 with idx1 = the lowest j that attains it, and the same from x2 to x1.  The distance is
//                       formed by the very expression of chamfer_min_kernel (pointops.hip: the reference's expanded form, the same fused
//                       multiply-adds), so d1 / d2 equal ldt_chamfer's outputs bit for bit; a strict `<` keeps the lowest index of a tie.
//   ldt_cd_loss         out = (loss, term1, term2), term = mean sqrt(max(d, 0)) (l1) or mean d (l2): float64 partials in index order, one
//                       workgroup, as ldt_sumsq's final stage.  (The expanded form can round a tiny distance below 0; the clamp keeps the
//                       root real.)
//   ldt_cd_loss_bwd     dx1[i] = w(i, idx1[i]) (x1_i - x2_idx1[i]) / (B n) + sum over {j : idx2[j] = i}, j ascending, of w(i, j) (x1_i - x2_j) / (B m),
//                       w = upstream / |x1_i - x2_j| (l1: 2 (x1 - x2) / (2 sqrt d)) or 2 upstream (l2).  The second sum is GATHERED: point i
//                       scans idx2 of its cloud, staged through LDS in tiles, so every element is summed by one thread in a fixed order: no
//                       atomics, the same bits on every run.
// Two deviations from the reference, both on purpose:
//   * a pair at distance exactly 0 contributes exactly 0 to the gradient.  Its direction vector is zero; the reference's 1 / (2 sqrt 0) is
//     inf and inf * 0 puts a NaN into every weight the gradient reaches.
//   * the l1 weight takes |x1_i - x2_j| from the difference vector the gradient already forms (three squares, one root: a few fp32 roundings,
//     RELATIVE), not from the stored d1 / d2, whose expanded form carries an ABSOLUTE error of 9 x 2^-24 (|x1|^2 + |x2|^2): for a close pair
//     that error is a large fraction of d, and 1 / sqrt(d) would carry it into the gradient.  chamfer3D.cu's distances are differences too.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define CDL_WG 256
#define CDL_TILE 2048                 // idx2 entries staged per LDS tile (8 KB); a multiple of 4

// one thread per query point; chamfer_min_kernel's loop with the index kept
__global__ __launch_bounds__(CDL_WG) void chamfer_nn_kernel(const float* __restrict__ q, const float* __restrict__ ref, int nq, int nr,
                                                            float* __restrict__ dist, int* __restrict__ idx) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * CDL_WG + threadIdx.x;
    if (i >= nq) return;
    const float* qp = q + ((long)b * nq + i) * 3;
    const float x = qp[0], y = qp[1], z = qp[2];
    const float qn = fmaf(z, z, fmaf(y, y, x * x));
    float m = INFINITY;
    int best = 0;
    const float* rp = ref + (long)b * nr * 3;
    for (int j = 0; j < nr; ++j) {
        const float rx = rp[3 * j], ry = rp[3 * j + 1], rz = rp[3 * j + 2];
        const float rn = fmaf(rz, rz, fmaf(ry, ry, rx * rx));
        const float dot = fmaf(z, rz, fmaf(y, ry, x * rx));
        const float d = (qn + rn) - 2.f * dot;
        if (d < m) { m = d; best = j; }
    }
    dist[(long)b * nq + i] = m;
    idx[(long)b * nq + i] = best;
}

extern "C" int ldt_chamfer_nn(const float* x1, const float* x2, int32_t B, int32_t n, int32_t m, float* d1, int32_t* idx1, float* d2,
                              int32_t* idx2, void* stream) {
    LDT_REQUIRE(x1 && x2 && d1 && idx1 && d2 && idx2, LDT_EARG, "chamfer_nn: null pointer");
    LDT_REQUIRE(B > 0 && B <= 65535 && n > 0 && m > 0, LDT_ESHAPE, "chamfer_nn: B %d (1 .. 65535), n %d, m %d", B, n, m);
    hipStream_t s = ldt_stream(stream);
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((unsigned)((n + CDL_WG - 1) / CDL_WG), (unsigned)B), dim3(CDL_WG), 0, s, x1, x2, n, m, d1, idx1);
    const int rc = ldt_check_launch("chamfer_nn (x1 -> x2)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((unsigned)((m + CDL_WG - 1) / CDL_WG), (unsigned)B), dim3(CDL_WG), 0, s, x2, x1, m, n, d2, idx2);
    return ldt_check_launch("chamfer_nn (x2 -> x1)");
}

// sum over the workgroup in a fixed order: lanes of a wave by halving, then the waves in index order.  Valid in thread 0.
__device__ __forceinline__ double cdl_block_sum(double v, double* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & (LDT_WAVE - 1)) == 0) part[threadIdx.x / LDT_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < CDL_WG / LDT_WAVE; ++w) s += part[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(CDL_WG) void cd_loss_kernel(const float* __restrict__ d1, long n1, const float* __restrict__ d2, long n2, int l1,
                                                         float* __restrict__ out) {
    __shared__ double part[CDL_WG / LDT_WAVE];
    double t[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const float* d = side ? d2 : d1;
        const long n = side ? n2 : n1;
        double acc = 0.0;
        for (long i = threadIdx.x; i < n; i += CDL_WG) {
            const double v = (double)d[i];
            acc += l1 ? sqrt(v > 0.0 ? v : 0.0) : v;
        }
        t[side] = cdl_block_sum(acc, part) / (double)n;
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(t[0] + t[1]);
        out[1] = (float)t[0];
        out[2] = (float)t[1];
    }
}

extern "C" int ldt_cd_loss(const float* d1, int64_t n1, const float* d2, int64_t n2, int32_t type, float* out, void* stream) {
    LDT_REQUIRE(d1 && d2 && out, LDT_EARG, "cd_loss: null pointer");
    LDT_REQUIRE(n1 > 0 && n2 > 0, LDT_ESHAPE, "cd_loss: %ld and %ld distances", (long)n1, (long)n2);
    LDT_REQUIRE(type == LDT_CD_L1 || type == LDT_CD_L2, LDT_EARG, "cd_loss: type %d is neither LDT_CD_L1 (1) nor LDT_CD_L2 (2)", type);
    hipLaunchKernelGGL(cd_loss_kernel, dim3(1), dim3(CDL_WG), 0, ldt_stream(stream), d1, (long)n1, d2, (long)n2,
                       (int)(type == LDT_CD_L1), out);
    return ldt_check_launch("cd_loss");
}

// one pair's term: w (p - r), w = c / |p - r| (l1) or c (l2); exactly 0 at distance 0
__device__ __forceinline__ void cdl_add_pair(float px, float py, float pz, const float* __restrict__ r, float c, int l1, float (&acc)[3]) {
    const float dx = px - r[0], dy = py - r[1], dz = pz - r[2];
    const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    if (dd == 0.f) return;
    const float w = l1 ? c / sqrtf(dd) : c;
    acc[0] = fmaf(w, dx, acc[0]); acc[1] = fmaf(w, dy, acc[1]); acc[2] = fmaf(w, dz, acc[2]);
}

// one thread per estimated point i of cloud blockIdx.y; the whole workgroup walks idx2 of the cloud tile by tile
__global__ __launch_bounds__(CDL_WG) void cd_loss_bwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const int* __restrict__ idx1,
                                                             const int* __restrict__ idx2, int n, int m, int l1, float c1, float c2,
                                                             float* __restrict__ dx1) {
    __shared__ __attribute__((aligned(16))) int tile[CDL_TILE];
    const int b = blockIdx.y;
    const int i = blockIdx.x * CDL_WG + threadIdx.x;
    const bool live = i < n;
    const float* r2 = x2 + (long)b * m * 3;
    float px = 0.f, py = 0.f, pz = 0.f, acc[3] = {0.f, 0.f, 0.f};
    if (live) {
        const float* p = x1 + ((long)b * n + i) * 3;
        px = p[0]; py = p[1]; pz = p[2];
        const int j = idx1[(long)b * n + i];
        if (j >= 0 && j < m) cdl_add_pair(px, py, pz, r2 + 3 * (long)j, c1, l1, acc);
    }
    const int* ib = idx2 + (long)b * m;
    for (int j0 = 0; j0 < m; j0 += CDL_TILE) {
        __syncthreads();
        for (int t = threadIdx.x; t < CDL_TILE; t += CDL_WG) tile[t] = j0 + t < m ? ib[j0 + t] : -1;     // -1 matches no point
        __syncthreads();
        if (live) {
            const int cnt = min(CDL_TILE, m - j0);
            for (int t = 0; t < cnt; t += 4) {                          // every lane reads the same 16 bytes: an LDS broadcast
                const int4 v = *reinterpret_cast<const int4*>(&tile[t]);
                if (v.x == i || v.y == i || v.z == i || v.w == i) {
                    if (v.x == i) cdl_add_pair(px, py, pz, r2 + 3 * (long)(j0 + t), c2, l1, acc);
                    if (v.y == i) cdl_add_pair(px, py, pz, r2 + 3 * (long)(j0 + t + 1), c2, l1, acc);
                    if (v.z == i) cdl_add_pair(px, py, pz, r2 + 3 * (long)(j0 + t + 2), c2, l1, acc);
                    if (v.w == i) cdl_add_pair(px, py, pz, r2 + 3 * (long)(j0 + t + 3), c2, l1, acc);
                }
            }
        }
    }
    if (live) {
        float* o = dx1 + ((long)b * n + i) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

extern "C" int ldt_cd_loss_bwd(const float* x1, const float* x2, const int32_t* idx1, const int32_t* idx2, int32_t B, int32_t n, int32_t m,
                               int32_t type, float upstream, float* dx1, void* stream) {
    LDT_REQUIRE(x1 && x2 && idx1 && idx2 && dx1, LDT_EARG, "cd_loss_bwd: null pointer");
    LDT_REQUIRE(B > 0 && B <= 65535 && n > 0 && m > 0, LDT_ESHAPE, "cd_loss_bwd: B %d (1 .. 65535), n %d, m %d", B, n, m);
    LDT_REQUIRE(type == LDT_CD_L1 || type == LDT_CD_L2, LDT_EARG, "cd_loss_bwd: type %d is neither LDT_CD_L1 (1) nor LDT_CD_L2 (2)", type);
    const int l1 = type == LDT_CD_L1;
    // l1: 2 (x1 - x2) / (2 sqrt d) = (x1 - x2) / |x1 - x2|;  l2: 2 (x1 - x2).  The means' 1 / (B n), 1 / (B m) and the upstream scalar in double
    const double f = (l1 ? 1.0 : 2.0) * (double)upstream;
    const float c1 = (float)(f / ((double)B * n)), c2 = (float)(f / ((double)B * m));
    hipLaunchKernelGGL(cd_loss_bwd_kernel, dim3((unsigned)((n + CDL_WG - 1) / CDL_WG), (unsigned)B), dim3(CDL_WG), 0,
                       ldt_stream(stream), x1, x2, idx1, idx2, n, m, l1, c1, c2, dx1);
    return ldt_check_launch("cd_loss_bwd");
}
