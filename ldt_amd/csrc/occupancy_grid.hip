// Occupancy histograms of the JSD metric (evaluation/evaluation_metrics.py:376-389 entropy_of_occupancy_grid): every point of every cloud
// is assigned to its nearest grid cell; counters[g] counts points, bernoulli[g] counts clouds with at least one point in g.
//   ldt_occupancy_grid   exact nearest cell by brute force, one workgroup per cloud.
// The reference asks sklearn's NearestNeighbors, whose tree works on float64 copies of the fp32 coordinates and accumulates the squared
// distance coordinate by coordinate: (dx^2 + dy^2) + dz^2 with every product and sum rounded (no FMA).  The same expression is evaluated
// here, cells in ascending index order with a strict "<", so the lowest index wins a tie.  Both histograms are integer: the adds commute,
// the result is exact and the same from run to run whatever order the atomics arrive in.
// Shape: a thread keeps OCC_PPT points in registers (float64), the cell list streams through LDS in tiles of OCC_TILE cells (float64, every
// lane reads the same address: a broadcast), 8 fp64 operations + a compare and two selects per (point, cell) pair: VALU-bound, 3 LDS reads
// per OCC_PPT pairs.  S = 1024 clouds x 2048 points x 11494 in-sphere cells of a 28^3 grid = 2.4e10 pairs.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define OCC_WG 256
#define OCC_PPT 8                     // points per thread and pass: 2048 points = one pass over the cells
#define OCC_TILE 512                  // cells per LDS tile (12 KB as float64)
#define OCC_MAX_CELLS 32768           // bits of the per-cloud de-duplication bitmap (4 KB); a 28^3 grid has 21952 cells, a 32^3 grid 32768

__device__ __forceinline__ double occ_dist2(double px, double py, double pz, double cx, double cy, double cz) {
#pragma clang fp contract(off)        // rounded products and sums, in the tree's order
    const double dx = px - cx;
    const double dy = py - cy;
    const double dz = pz - cz;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz;
}

__global__ __launch_bounds__(OCC_WG) void occupancy_grid_kernel(const float* __restrict__ pts, int n, const float* __restrict__ cells, int G,
                                                                uint32_t* __restrict__ counters, uint32_t* __restrict__ bernoulli) {
    __shared__ double tile[OCC_TILE * 3];
    __shared__ uint32_t seen[OCC_MAX_CELLS / 32];
    const float* p = pts + (long)blockIdx.x * n * 3;
    for (int w = threadIdx.x; w < (G + 31) / 32; w += OCC_WG) seen[w] = 0u;         // (made visible by the first barrier below)
    for (int base = 0; base < n; base += OCC_WG * OCC_PPT) {
        double px[OCC_PPT], py[OCC_PPT], pz[OCC_PPT], best[OCC_PPT];
        int arg[OCC_PPT];
#pragma unroll
        for (int k = 0; k < OCC_PPT; ++k) {
            const int i = base + k * OCC_WG + (int)threadIdx.x;
            const bool valid = i < n;
            px[k] = valid ? (double)p[3 * (long)i] : 0.0;
            py[k] = valid ? (double)p[3 * (long)i + 1] : 0.0;
            pz[k] = valid ? (double)p[3 * (long)i + 2] : 0.0;
            best[k] = __builtin_huge_val();
            arg[k] = 0;                                                               // (a NaN point never compares below: cell 0, in bounds)
        }
        for (int c0 = 0; c0 < G; c0 += OCC_TILE) {
            const int m = min(OCC_TILE, G - c0);
            __syncthreads();                                                          // the previous tile has been read by every wave
            for (int j = threadIdx.x; j < 3 * m; j += OCC_WG) tile[j] = (double)cells[3 * (long)c0 + j];
            __syncthreads();
            for (int c = 0; c < m; ++c) {
                const double cx = tile[3 * c], cy = tile[3 * c + 1], cz = tile[3 * c + 2];
#pragma unroll
                for (int k = 0; k < OCC_PPT; ++k) {
                    const double d = occ_dist2(px[k], py[k], pz[k], cx, cy, cz);
                    const bool lower = d < best[k];
                    best[k] = lower ? d : best[k];
                    arg[k] = lower ? c0 + c : arg[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < OCC_PPT; ++k) {
            if (base + k * OCC_WG + (int)threadIdx.x < n) {
                const int g = arg[k];                                                 // 0 <= g < G
                atomicAdd(&counters[g], 1u);
                const uint32_t bit = 1u << (g & 31);
                const uint32_t old = atomicOr(&seen[g >> 5], bit);                   // exactly one point of the cloud finds the bit clear
                if (!(old & bit)) atomicAdd(&bernoulli[g], 1u);
            }
        }
    }
}

extern "C" int ldt_occupancy_grid(const float* pts, int32_t S, int32_t n, const float* cells, int32_t G, uint32_t* counters, uint32_t* bernoulli,
                                  void* stream) {
    LDT_REQUIRE(pts && cells && counters && bernoulli, LDT_EARG, "occupancy_grid: null pointer");
    LDT_REQUIRE(S > 0 && n > 0 && G > 0 && G <= OCC_MAX_CELLS && (long)n * 3 <= 0x7fffffffL, LDT_ESHAPE,
                "occupancy_grid: S %d clouds of n %d points, G %d cells (1..%d)", S, n, G, OCC_MAX_CELLS);
    hipLaunchKernelGGL(occupancy_grid_kernel, dim3((unsigned)S), dim3(OCC_WG), 0, ldt_stream(stream), pts, n, cells, G, counters,
                       bernoulli);
    return ldt_check_launch("occupancy_grid");
}
