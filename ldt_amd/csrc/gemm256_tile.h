// The 256-row-tile GEMM machinery shared by gemm_256.hip's two kernels (gfx950), plus the host's view of their tile list.
//
// gemm_bf16_nt_256f_kernel: persistent 256 x 256 tiles, one workgroup per CU, K streamed continuously ACROSS the workgroup's tiles.
// gemm_qkv_attn256_kernel: the same main loop on 256 x 192 tiles ([q | k | v] of one head), attention in the epilogue.
//
//   * 512 threads = 8 waves; wave w and w + 4 share a SIMD.  Group grp = w >> 2 owns output rows [128 grp, +128) of the tile, wn = w & 3 a
//     band of its columns (64, or 48 of 192): per wave 8 x NF accumulator tiles of mfma_f32_16x16x32_bf16, NF = 4 or 3 W fragments per
//     k-half, operands swapped (D[n][m] = W . X^T: a lane ends up with 4 consecutive output columns of one row).
//   * LDS map (G256_*): two operand buffers of 64 KiB, each X[256][64] at + 0 | W[<= 256][64] at + G256_W_OFF, bf16 rows of 128 B whose 16-B
//     chunk index is XORed with (row >> 1) & 7 (conflict-free ds_read_b128 of 16 x 32 fragments; applied on the DMA source address and on
//     the read address); behind them one 4 KiB staging area per wave (epilogue rows; its tail holds the LN-fold statistics and S | C slices).
//   * Operands arrive by LDS-DMA in pieces of 8 rows x 128 B — whole lines: every line of X / W is requested once (Stream256).  Addresses
//     are a wave-uniform base (tile origin + k, SGPRs) plus per-lane 32-bit offsets that never change, so the stream advance is scalar.
//     The stream does not stop at a tile boundary: behind a tile's last K-tile it continues with the workgroup's next tile; behind the
//     last tile it parks (re-requests the last K-tile, never consumed).
//   * A 64-deep K-tile = two 32-deep k-halves = four phases p0..p3 (ktile256): [ds_reads of the phase's operands + the caller's requests
//     and counted wait] barrier [4 NF MFMAs] barrier.  Group 1 runs one barrier behind group 0, so on every SIMD one wave issues MFMAs while
//     its partner reads LDS / issues DMA.  During K-tile s the next one is requested into the other buffer, part by part as its rows retire:
//     p0: W(s+1)    p1: X rows {0..63, 128..191}(s+1) ("xa", 2 pieces per wave)    p2: the other X rows ("xb", 2 pieces).
//   * Counted waits (VMEM retires in order: vmcnt(N) = N younger requests may be in flight): p0 waits for this K-tile's xb (read in p1), p3
//     for W and xa of s+1 (read in the next p0).  Both sit before the phase's first barrier; the reads they cover come two barriers later.
//     The first waits after an epilogue allow for the epilogue's own stores.  Each kernel states its own counts beside its requests.
//   * Epilogues (g256_epilogue_staged): accumulators -> the wave's staging area -> 16 B per lane over whole output rows (the raw fragment
//     layout is store-issue bound); stores are not waited for, they drain under the next tile's main loop.
// Interior, aligned tiles only (ldt_gemm256_takes).
#pragma once
#include <type_traits>

#include "kernels.h"

enum { FOLD_NONE = 0, FOLD_PRODUCER = 1, FOLD_CONSUMER = 2 };   // LN folding (below)

// ---- LDS map
#define G256_BUF_BYTES 65536                               /* one operand buffer: X | W of one K-tile */
#define G256_W_OFF 32768                                   /* W inside a buffer */
#define G256_RING_BYTES (2 * G256_BUF_BYTES)               /* both buffers; XRING reuses them as eight 16 KiB residual rings */
#define G256_LDS_BYTES (G256_RING_BYTES + 8 * 4096)        /* + one 4 KiB staging area per wave = 160 KiB */
#define G256_STATS_OFF 2304                                /* staging area: bf16 rows use 16 x 144 B; then 1 KiB of row statistics */
#define G256_SC_OFF (G256_STATS_OFF + 1024)                /* 512 B: a 128-column slice of fold_S (waves 0, 1) or fold_C (waves 2, 3) */

#define G256_BARRIER()                        \
    do {                                      \
        __builtin_amdgcn_sched_barrier(0);    \
        __builtin_amdgcn_s_barrier();         \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)

// ---- THE tile list: which tiles workgroup `bid` of a grid of G computes, and in which order.  The tile ids 0 .. tiles - 1 are cut into
// min(G, 8) contiguous chunks, one per XCD label (workgroups b, b + 8, ... share an XCD's L2); the workgroups of a label take their chunk's
// ids round-robin.  An id is a position in the grouped sweep: group_m row panels x every column tile, column by column (group_m <= 1:
// row-major).  Both kernels and ldt_gemm_decide read this one definition: "one tile per workgroup" is max_count() == 1, nothing else.
struct Tile256List {
    int tiles_m, tiles_n, gm;
    int c_lo, j, stride, count;                                          // ids c_lo + j + i * stride, i < count
    __host__ __device__ Tile256List(int tiles_m_, int tiles_n_, int group_m, int G, int bid) : tiles_m(tiles_m_), tiles_n(tiles_n_), gm(group_m) {
        const int tiles = tiles_m * tiles_n;
        const int nx = G < 8 ? G : 8;
        const int xcd = bid % nx;
        j = bid / nx;
        stride = (G - xcd + nx - 1) / nx;                                // workgroups of this label
        const int c_hi = (int)((long)tiles * (xcd + 1) / nx);
        c_lo = (int)((long)tiles * xcd / nx);
        count = (c_hi - c_lo - j + stride - 1) / stride > 0 ? (c_hi - c_lo - j + stride - 1) / stride : 0;
    }
    __host__ __device__ void tile(int i, int& tm, int& tn) const {
        const int id = c_lo + j + i * stride;
        if (gm <= 1) { tm = id / tiles_n; tn = id % tiles_n; return; }
        const int per = gm * tiles_n, g = id / per, r = id - g * per;
        const int rows = gm < tiles_m - g * gm ? gm : tiles_m - g * gm;
        tm = g * gm + r % rows; tn = r / rows;
    }
    // most tiles any workgroup of the grid computes (a label's counts fall with j: its first workgroup has the most)
    static int max_count(int tiles_m, int tiles_n, int G) {
        int mx = 0;
        for (int b = 0; b < G && b < 8; ++b) { const int c = Tile256List(tiles_m, tiles_n, 1, G, b).count; mx = c > mx ? c : mx; }
        return mx;
    }
};

// ---- host side (gemm_256.hip unless noted)
// rows per group of the tile order: wide outputs (QKV: 12 column tiles, MLP-up: 16) are swept in groups of 4 row panels, so an XCD's 32
// workgroups hold a 4 x 8 block of tiles in its 4 MiB L2 instead of 2 x 16 — the W panel set is then re-streamed from the fabric once per
// group, not once per 2 row panels (profiles/r06_tile_order_sweep.txt: 8 / 4 / 1 row panels = 10.76-10.79 / 10.59-10.64 / 10.56-10.60 ms per
// SDE step with the fused QKV + attention kernel and the LN-folded MLP-up in place)
static inline int gemm256_default_group_m(int tiles_m, int tiles_n) { return (tiles_n >= 8 && tiles_m >= 8) ? 4 : 1; }
bool ldt_gemm256_takes(int epi, const GemmArgs* a);       // interior, aligned tiles only: everything else belongs to the mid-size / small-tile kernels
int ldt_gemm256_launch(int epi, int fold, const GemmArgs* a, const GemmRoute& route, hipStream_t stream);   // route: ldt_gemm_decide's (a 256 family)

// sum over the 16 lanes of a DPP row (all 16 end up with the total): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// LN folding (FOLD): the LayerNorm + AdaLN modulate between a residual GEMM and the next projection never runs as a
// kernel.  With h = LN(x)(1 + sc) + sh, r = rstd(x), mu = mean(x):
//     h . W^T + b  =  r * ( xs . W^T )  -  r * mu * S  +  C,     xs = x (1 + sc),  S_n = sum_k (1 + sc_k) W_nk,  C_n = sum_k sh_k W_nk + b_n
//   FOLD_PRODUCER (EPI_RESID_F32): besides x_new the epilogue stores xs = bf16(x_new (1 + sc)) and, per row, the partial
//     (sum, sum of squares) of x_new over this tile's 256 columns  -> stats_out[n0/256][M][2]  (DPP row sums, the four
//     column waves combined through LDS: one 8-B value per row and tile, summed in a fixed order — no atomics).
//   FOLD_CONSUMER (EPI_BF16 / EPI_GELU_BF16): X = xs; the tile's 256 rows x stats_parts partials are fetched by one
//     LDS-DMA piece per wave during the main loop (into the unused tail of the bf16 staging areas), r / -r mu are
//     formed per lane at the start of the epilogue and y = r acc + (-r mu S + C) replaces acc + bias.
//   S, C are batch-invariant per-step tables built by the host in fp32 from the same bf16 W the MFMAs read; they are
//   step-indexed, hence cold in every cache at every step: the tile's two 1 KiB slices ride the same mid-loop DMA slot
//   (four half-wave pieces) so that the epilogue opens on LDS reads instead of an HBM round trip.  For the same reason
//   the residual epilogue's step-indexed gate / ln_scale vectors of a workgroup's first tile are loaded before the
//   main loop and kept in 8 VGPRs.

// FOLD_CONSUMER, once per tile and off the epilogue's critical path: thread R < 256 adds row R's partial (sum, sumsq)
// pairs (piece part*2 + (R >> 7) sits in that wave's staging tail) and overwrites the part-0 slot with (rstd, -mean*rstd).
__device__ __forceinline__ void g256_fold_finalize(char* stage_base, int R, int parts, int K) {
    char* slot = stage_base + (R >> 7) * 4096 + G256_STATS_OFF + (R & 127) * 8;
    float s1 = 0.f, s2 = 0.f;
    for (int pp = 0; pp < parts; ++pp) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(slot + pp * 2 * 4096);
        s1 += t[0]; s2 += t[1];
    }
    const float invk = 1.0f / (float)K;
    const float mean = s1 * invk;
    const float var = fmaxf(s2 * invk - mean * mean, 0.f);
    const float r = rsqrtf(var + 1e-6f);
    *reinterpret_cast<f32x2*>(slot) = (f32x2){r, -mean * r};
}

// interior tiles: per-wave LDS staging (16 output rows per pass) -> 16 B per lane over whole rows
// XRING (EPI_RESID_F32 on a workgroup's LAST tile, batch-shared gate): the fp32 residual rows are not loaded pass by pass into
// VGPRs (4 x 16 B per lane in flight per wave = 32 KB per CU: at ~2.5 us of HBM latency that caps the read at ~3.3 TB/s
// chip-wide, 18-21 us of exposed epilogue — tools/dbg/epi_ablate.py) but by LDS-DMA into the operand ring, which is idle by
// then: `xring` = this wave's 16 KiB of it = four 4 KiB pass slots.  Passes 0..3 are requested up front, pass mi + 4 when
// pass mi has consumed its slot: 16 KB per wave (128 KB per CU) in flight, lane-linear both ways (a lane reads back the 16 B it
// requested).  Counted waits: vmcnt(N), N = the ops issued after pass mi's requests (later requests + SP stores per pass).
template <int EPI, int FOLD, int XRING = 0>
__device__ __forceinline__ void g256_epilogue_staged(const GemmArgs& a, f32x4 (&acc)[4][8], int m0, int n0, int grp, int wn,
                                                   int lane, int lrow, int lchk, const float* gate, char* reg, char* stage_base,
                                                   const float* ln_scale, bool have_pre, f32x4 g4_pre, f32x4 sc4_pre,
                                                   char* xring = nullptr) {
    const int mb = m0 + grp * 128, nb = n0 + wn * 64;
    f32x4 bias4[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
        bias4[ni] = (a.bias && FOLD != FOLD_CONSUMER) ? *reinterpret_cast<const f32x4*>(a.bias + nb + ni * 16 + lchk * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_RELU_BF16) {
        constexpr int RS = 128 + 16;                              // staged row: 64 bf16 + 16 B pad
        f32x4 s4[4];
        float rr[8], nm[8];
        if (FOLD == FOLD_CONSUMER) {
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {                      // (rstd, -mean*rstd) of the lane's rows, finalised mid-loop (g256_fold_finalize)
                const int R = grp * 128 + mi * 16 + lrow;
                const f32x2 t = *reinterpret_cast<const f32x2*>(stage_base + (R >> 7) * 4096 + G256_STATS_OFF + (R & 127) * 8);
                rr[mi] = t[0]; nm[mi] = t[1];
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int c = wn * 64 + ni * 16 + lchk * 4;       // S | C slices of this tile: DMA'd into waves 0..3's areas
                s4[ni] = *reinterpret_cast<const f32x4*>(stage_base + (c >> 7) * 4096 + G256_SC_OFF + (c & 127) * 4);
                bias4[ni] = *reinterpret_cast<const f32x4*>(stage_base + (2 + (c >> 7)) * 4096 + G256_SC_OFF + (c & 127) * 4);
            }
        }
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                f32x4 v = acc[ni][mi];
                if (FOLD == FOLD_CONSUMER) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] * rr[mi] + (nm[mi] * s4[ni][r] + bias4[ni][r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += bias4[ni][r];
                }
                if (EPI == EPI_GELU_BF16) {
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {                 // two lanes of the polynomial per v_pk_* instruction
                        const f32x2 gg = gelu_erf_fast2((f32x2){v[r], v[r + 1]});
                        v[r] = gg[0]; v[r + 1] = gg[1];
                    }
                }
                if (EPI == EPI_RELU_BF16) {
                    if (a.skip) {
                        const bf16x4 sk = *reinterpret_cast<const bf16x4*>(a.skip + (long)(mb + mi * 16 + lrow) * a.lds_ + nb + ni * 16 + lchk * 4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += (float)sk[r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                }
                const bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                *reinterpret_cast<bf16x4*>(reg + lrow * RS + (ni * 16 + lchk * 4) * 2) = pk;
            }
            bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + (long)(mb + mi * 16) * a.ldo + nb;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                const bf16x8 d = *reinterpret_cast<const bf16x8*>(reg + row * RS + ch * 16);
                *reinterpret_cast<bf16x8*>(o + (long)row * a.ldo + ch * 8) = d;
            }
        }
    } else {
        const int ch = lane & 15;                                 // 16-B chunk of the 256-B fp32 row (XOR-swizzled by row)
        f32x4 g4 = {1.f, 1.f, 1.f, 1.f};
        const bool has_gate = (EPI == EPI_RESID_F32) && gate;
        const bool shared_gate = has_gate && a.gate_sample_stride == 0;
        if (shared_gate) g4 = have_pre ? g4_pre : *reinterpret_cast<const f32x4*>(gate + nb + ch * 4);
        f32x4 sc4 = {1.f, 1.f, 1.f, 1.f};
        constexpr int SP = (FOLD == FOLD_PRODUCER) ? 8 : 4;       // VMEM stores a pass issues (x, and xs for the producer)
        // running source pointer: row (lane>>4) of the next 4-row group, advanced 4 rows per request (passes are requested in
        // order 0..7); kept opaque so that hipcc does not materialise all 32 addresses up front
        const float* xsrc = XRING ? a.resid + ((long)mb + (lane >> 4)) * a.ldr + nb + ch * 4 : nullptr;
        const long xstep = (long)4 * a.ldr;
        auto request_pass = [&](int p) {                          // 4 x 1 KiB: rows it*4 + (lane>>4) of pass p, 16 B per lane
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xsrc,
                                                 (__attribute__((address_space(3))) void*)(xring + (p & 3) * 4096 + it * 1024), 16, 0, 0);
                xsrc += xstep;
                asm volatile("" : "+v"(xsrc));
            }
        };
        if (XRING) { request_pass(0); request_pass(1); request_pass(2); request_pass(3); }
        float rs1[8], rs2[8];                                     // FOLD_PRODUCER: lanes with (lane & 15) < 4 keep row (lane&15)*4 + (lane>>4) of pass mi
        if (FOLD == FOLD_PRODUCER) {
            const f32x4 t = have_pre ? sc4_pre : *reinterpret_cast<const f32x4*>(ln_scale + nb + ch * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) sc4[r] = 1.0f + t[r];
        }
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                f32x4 v = acc[ni][mi];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += bias4[ni][r];
                *reinterpret_cast<f32x4*>(reg + lrow * 256 + (((ni * 4 + lchk) ^ lrow) << 4)) = v;
            }
            const long mrow0 = mb + mi * 16;
            float k1 = 0.f, k2 = 0.f;
            if (XRING) {                                             // pass mi's rows have landed (ops issued after its requests: see above)
                constexpr int NW[8] = {12, 12 + SP, 12 + 2 * SP, 12 + 3 * SP, 12 + 3 * SP, 8 + 3 * SP, 4 + 3 * SP, 3 * SP};
                switch (mi) {                                        // (mi is a compile-time constant of the unrolled loop)
                    case 0: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[0]) : "memory"); break;
                    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[1]) : "memory"); break;
                    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[2]) : "memory"); break;
                    case 3: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[3]) : "memory"); break;
                    case 4: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[4]) : "memory"); break;
                    case 5: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[5]) : "memory"); break;
                    case 6: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[6]) : "memory"); break;
                    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NW[7]) : "memory"); break;
                }
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 4 + (lane >> 4);
                f32x4 v = *reinterpret_cast<const f32x4*>(reg + row * 256 + ((ch ^ row) << 4));
                float* o = reinterpret_cast<float*>(a.out) + (mrow0 + row) * a.ldo + nb + ch * 4;
                if (EPI == EPI_RESID_F32 && XRING) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(xring + (mi & 3) * 4096 + it * 1024 + lane * 16);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = x[r] + g4[r] * v[r];
                } else if (EPI == EPI_RESID_F32) {
                    f32x4 x = {0.f, 0.f, 0.f, 0.f};
                    if (!(a.dbg & 1)) x = *reinterpret_cast<const f32x4*>(a.resid + (mrow0 + row) * a.ldr + nb + ch * 4);
                    if (has_gate && !shared_gate)
                        g4 = *reinterpret_cast<const f32x4*>(gate + ((mrow0 + row) / a.rows_per_sample) * a.gate_sample_stride + nb + ch * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = x[r] + g4[r] * v[r];
                }
                if (XRING || !(a.dbg & 2)) *reinterpret_cast<f32x4*>(o) = v;
                if (FOLD == FOLD_PRODUCER) {
                    const bf16x4 pk = {(bf16_t)(v[0] * sc4[0]), (bf16_t)(v[1] * sc4[1]), (bf16_t)(v[2] * sc4[2]), (bf16_t)(v[3] * sc4[3])};
                    if (XRING || !(a.dbg & 4)) *reinterpret_cast<bf16x4*>(a.xs + (mrow0 + row) * a.ldxs + nb + ch * 4) = pk;
                    const float s1 = row16_sum((v[0] + v[1]) + (v[2] + v[3]));
                    const float s2 = row16_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
                    const bool keep = (lane & 15) == it;
                    k1 = keep ? s1 : k1; k2 = keep ? s2 : k2;
                }
            }
            rs1[mi] = k1; rs2[mi] = k2;
            if (XRING && mi < 4) request_pass(mi + 4);               // into the slot this pass has just consumed
        }
        if (FOLD == FOLD_PRODUCER && !(a.dbg & 8)) {
            // the wave's 128 rows x (sum, sumsq) over its 64 columns -> head of its staging area; the four column waves of a
            // row group are then added in the fixed order wn = 0..3 by one thread per row
            if ((lane & 15) < 4) {
#pragma unroll
                for (int mi = 0; mi < 8; ++mi)
                    *reinterpret_cast<f32x2*>(reg + (mi * 16 + (lane & 15) * 4 + (lane >> 4)) * 8) = (f32x2){rs1[mi], rs2[mi]};
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G256_BARRIER();
            const int tid = threadIdx.x;
            if (tid < 256) {
                const char* src = stage_base + (tid >> 7) * 4 * 4096 + (tid & 127) * 8;
                f32x2 t = *reinterpret_cast<const f32x2*>(src);
#pragma unroll
                for (int w = 1; w < 4; ++w) { const f32x2 u = *reinterpret_cast<const f32x2*>(src + w * 4096); t[0] += u[0]; t[1] += u[1]; }
                *reinterpret_cast<f32x2*>(a.stats_out + ((long)(n0 >> 8) * a.M + m0 + tid) * 2) = t;
            }
        }                                                         // (the staging areas are next written a whole main loop later)
    }
}

// =================================================================================================
// The operand stream of one wave: X as 2 + 2 pieces per K-tile (xa: tile rows 0..63 and 128..191 = m-tiles 0-3 of the two groups, xb: the
// rows 64 below them), W as NWP pieces whose offsets the kernel fills in (wvo: global bytes from the tile's first W row; wds: LDS bytes
// inside a buffer).  piece = 8 rows x 128 B: lane -> row (lane >> 3) of the piece, LDS position lane & 7 holds chunk (lane & 7) ^ ((row >> 1) & 7).
// W_TILE_ROWS: rows of W between two column tiles (256; 64 = one head of the fused QKV tile, whose three segments lie `hidden` apart).
template <int NWP, int W_TILE_ROWS>
struct Stream256 {
    int wvo[NWP], xavo[2], xbvo[2];                                      // per-lane global byte offsets from the (tile row 0, k) element
    int wds[NWP], xads[2], xbds[2];                                      // LDS byte offsets inside a buffer (wave-uniform)
    const char* sxb = nullptr;                                           // stream bases: X / W at the stream's (tile, K-tile)
    const char* swb = nullptr;
    int s_it = 0, s_kt = 0, s_inc = 128;                                 // tile iteration, K-tile inside it, bytes per advance (0 once parked)

    __device__ __forceinline__ Stream256(const GemmArgs& a, int wave, int lane) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int pj = wave * 2 + q;                                 // 0..15: rows 0..63 then 128..191
            const int r0 = pj < 8 ? pj * 8 : 128 + (pj - 8) * 8;
            const int ra = r0 + (lane >> 3), rb = ra + 64;
            xavo[q] = ra * (int)a.ldx * 2 + (((lane & 7) ^ ((ra >> 1) & 7)) << 4);
            xbvo[q] = rb * (int)a.ldx * 2 + (((lane & 7) ^ ((rb >> 1) & 7)) << 4);
            xads[q] = r0 * 128;
            xbds[q] = (r0 + 64) * 128;
        }
    }
    __device__ __forceinline__ void seek(const GemmArgs& a, const Tile256List& tl, int it) {
        int tm, tn;
        tl.tile(it, tm, tn);
        sxb = reinterpret_cast<const char*>(a.X + (long)(tm * 256) * a.ldx);
        swb = reinterpret_cast<const char*>(a.W + (long)tn * W_TILE_ROWS * a.ldw);
    }
    __device__ __forceinline__ void advance(const GemmArgs& a, const Tile256List& tl) {   // after the last part (xb) of a K-tile was requested
        sxb += s_inc; swb += s_inc;
        if (++s_kt == (a.K >> 6)) {
            s_kt = 0;
            if (++s_it < tl.count) seek(a, tl, s_it);
            else { sxb -= s_inc; swb -= s_inc; s_inc = 0; s_kt = -0x40000000; }   // parked: re-reads the last K-tile, never consumed
        }
    }
    static __device__ __forceinline__ void piece(const char* src, char* dst) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
    __device__ __forceinline__ void issue_w(char* buf) const {
#pragma unroll
        for (int q = 0; q < NWP; ++q) piece(swb + wvo[q], buf + wds[q]);
    }
    __device__ __forceinline__ void issue_xa(char* buf) const {
#pragma unroll
        for (int q = 0; q < 2; ++q) piece(sxb + xavo[q], buf + xads[q]);
    }
    __device__ __forceinline__ void issue_xb(char* buf) const {
#pragma unroll
        for (int q = 0; q < 2; ++q) piece(sxb + xbvo[q], buf + xbds[q]);
    }
};

// per-lane LDS read bases inside a buffer: row * 128 + ((k-half * 4 + lchk) ^ ((row >> 1) & 7)) * 16; fragment i at + i * 2048.
// wcol0: the wave's first tile column (= row of the W image)
struct KTileLanes {
    int xb[2], wb[2];
    __device__ __forceinline__ KTileLanes(int grp, int wcol0, int lrow, int lchk) {
        const int sw = (lrow >> 1) & 7;
        const int xrb = (grp * 128 + lrow) * 128, wrb = G256_W_OFF + (wcol0 + lrow) * 128;
        xb[0] = xrb + ((lchk ^ sw) << 4); xb[1] = xrb + (((4 + lchk) ^ sw) << 4);
        wb[0] = wrb + ((lchk ^ sw) << 4); wb[1] = wrb + (((4 + lchk) ^ sw) << 4);
    }
};

// One K-tile out of buffer `st`: phase PH = 2 * k-half + m-half multiplies the k-half's NF W fragments with X m-tiles [4 m-half, +4).
//   request(Phase<PH>)   before the phase's first barrier, behind its LDS reads: the caller's DMA requests and counted wait
template <int PH> using Phase = std::integral_constant<int, PH>;
template <int NF, class Req>
__device__ __forceinline__ void ktile256(const char* st, const KTileLanes& ln, f32x4 (&acc)[NF][8], Req&& request) {
    bf16x8 wf[NF], xf[4];
    auto phase = [&](auto ph) {
        constexpr int PH = decltype(ph)::value, KH = PH >> 1, MH = PH & 1;
        if constexpr (MH == 0) {
#pragma unroll
            for (int i = 0; i < NF; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(st + ln.wb[KH] + i * 2048);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(st + ln.xb[KH] + (MH * 4 + i) * 2048);
        request(ph);
        G256_BARRIER();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < NF; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][MH * 4 + mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], xf[mi], acc[ni][MH * 4 + mi], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        G256_BARRIER();
    };
    phase(Phase<0>{}); phase(Phase<1>{}); phase(Phase<2>{}); phase(Phase<3>{});
}

// LN-fold consumer, mid-loop: this tile's 256 rows x stats_parts statistics partials, one LDS-DMA piece per wave -> its staging tail
__device__ __forceinline__ void g256_fold_stats_dma(const GemmArgs& a, int m0, int wave, int lane, char* stage_reg) {
    if (wave < 2 * a.stats_parts) {
        const float* src = a.stats_in + ((long)(wave >> 1) * a.M + m0 + (wave & 1) * 128) * 2 + lane * 4;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stage_reg + G256_STATS_OFF), 16, 0, 0);
    }
}
