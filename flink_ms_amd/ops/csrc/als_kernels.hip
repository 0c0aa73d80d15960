// ALS hot-path kernels for MI355X (gfx950, CDNA4).
//
// Rebuilds the compute core of flink-ml's blocked ALS (driven by the
// reference's flink-als/src/main/scala/de/tub/it4bi/ALSImpl.scala:47-52) as
// MI355X-native HIP:
//
//   K1  per-entity normal equations  A_u = sum_{i in R(u)} q_i q_i^T
//       + lambda*n_u*I,  b_u = sum r_ui q_i
//       -> MFMA rank-32 updates: the entity's rated factor rows are staged
//          through LDS in 32-row chunks and contracted with
//          v_mfma_f32_16x16x32_bf16 into 16x16 fp32 accumulator tiles
//          (upper triangle only; A is symmetric).  The rating value rides in
//          an extra staged 16-column block as a bf16 hi/lo pair, so b falls
//          out of the same MFMAs (columns 0/1 of the EXT tiles).
//   K2  p_u = A_u^{-1} b_u
//       -> LDL^T factorization (register panels + f32-MFMA trailing
//          updates) and substitution solves: wave-per-entity for k <= 64
//          (k_ldl_solve_wave_reg, A in MFMA C-fragments; fused with K1 in
//          k_als_solve_wavefused) or 256-thread blocks up to k = 128
//          (cholesky_lds_tri/solve_lds_block_tri over an LDS image, fused
//          with K1 in k_als_solve_fused) -- fused, A never round-trips
//          through HBM.
//
// Every Gramian kernel is templated on <KT, FP8>: factor rank k = 16*KT
// (KT 1..8, wrappers pad) and the gather precision (bf16 words or e4m3
// bytes); everything downstream of the MFMAs is fp32 either way.
//
// Block-path geometry: one workgroup (256 threads = 4 waves) per entity;
// grid = #entities; wave w owns accumulator tiles t = w, w+4, ... of the
// upper-triangle + EXT tile list.
//
// LDS layout per block (union; the stage dies before A is born):
//   stage: TRANSPOSED Gt[K+16 rows][32 ratings], one buffer per chunk in
//          flight.  bf16: 96-B row stride (24 dwords: 16 used + 8 pad),
//          one ds_read_b128 per MFMA fragment; e4m3: 40-B stride, one
//          ds_read_b64.  Rows 0..K-1 hold the gathered factor columns,
//          rows K..K+1 the rating hi/lo pair, K+2..K+15 zeros; staging
//          transposes in registers (als_kernels_device.inc).
//   A:     solver image (k_als_solve_fused, k_cholesky_solve): the
//          KT(KT+1)/2 lower-triangle 16x16 fp32 tiles, row stride 17
//          (Geo::LDT; conflict-free column walks), then b_hi/b_lo and the
//          substitution's x buffer, [K] fp32 each.
//          k_gramian, which only exports A, keeps the square [K][K+1]
//          image (write_acc mirrors the upper tiles into it).
//
// File layout: kernels first (block path, wave solvers, wave-fused, MFMA
// probes), then every extern "C" launcher declared in fma_api.h.

#include "common.hip.h"

#include "als_kernels_device.inc"
#include "fma_api.h"

// -------------------------------------------------------------- kernels

// Fused K1+K2: normal equations + LDL^T solve, one entity per block.
// FP8 selects the gather precision and, with it, the low-precision image of
// the solution written beside out_f32 for the next half-iteration (bf16
// words or e4m3 bytes; out_lowp may be null).
//
// WT (every Gramian kernel below): the weighted normal equations of
// confidence-weighted (implicit-feedback) ALS,
//   A = G0 + sum_j row~_j row~_j^T + reg*n*I,  b = sum_j pair(ext_j) row~_j,
//   row~_j = round_D(scale_j * F[indices_j]),
// with ``values`` carrying ext[], ``scale`` the per-rating sqrt-weights and
// ``G0`` the symmetric [K][K] fp32 base matrix (lower triangle read).  The
// WT = false instantiations ignore scale / G0 (null) and compile to what
// they compiled to before the flag existed.
template <int KT, bool FP8, bool WT = false>
__launch_bounds__(256)
// waves_per_eu(3): without it the allocator splits 93 VGPR + 88 AGPR
// (181 total -> 2 waves/SIMD); constrained it finds a 127-VGPR, zero-AGPR,
// zero-spill allocation -> 3-4 waves/SIMD (measured: the K=128 fused
// kernel is the whole 1B-config iteration)
__attribute__((amdgpu_waves_per_eu(3)))
__global__ void k_als_solve_fused(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ values,
    const typename GatherT<FP8>::elem* __restrict__ factors,
    float* __restrict__ out_f32,
    typename GatherT<FP8>::elem* __restrict__ out_lowp,
    const int* __restrict__ row_order, long long nrows, float reg,
    const float* __restrict__ scale, const float* __restrict__ G0) {
    constexpr int K = Geo<KT>::K;
    __shared__ __align__(16) char
        smem[FP8 ? Geo<KT>::SMEM8_TRI : Geo<KT>::SMEM_TRI];
    long long row = blockIdx.x;
    if (row >= nrows) return;
    if (row_order) row = row_order[row];

    const int n = gramian_to_lds<KT, true, true, FP8, WT>(
        smem, indptr, indices, values, factors, row, reg, scale, G0);
    if (n == 0) { write_zero_row<KT>(out_f32, out_lowp, row); return; }

    float* A = (float*)smem;
    float* b = A + Geo<KT>::A_TRI_FLOATS;
    cholesky_lds_tri<K>(A);
    // the solver takes one pointer per image format (k_cholesky_solve
    // passes neither); each instantiation here hands it exactly one
    if constexpr (FP8)
        solve_lds_block_tri<K>(A, b, b + 2 * K, out_f32 + row * K, nullptr,
                               out_lowp ? out_lowp + row * K : nullptr);
    else
        solve_lds_block_tri<K>(A, b, b + 2 * K, out_f32 + row * K,
                               out_lowp ? out_lowp + row * K : nullptr);
}

// Standalone K1 (for parity tests / modular path): writes dense A and b.
// row_order (optional): degree-descending launch schedule — block i
// processes entity row_order[i] and writes A_out/b_out at THAT row, so the
// downstream batched solve stays order-agnostic (heavy entities launch
// first; avoids tail stragglers at the end of the grid).
template <int KT, bool FP8, bool WT = false>
__launch_bounds__(256)
__global__ void k_gramian(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ values,
    const typename GatherT<FP8>::elem* __restrict__ factors,
    float* __restrict__ A_out,   // [nrows][K][K]
    float* __restrict__ b_out,   // [nrows][K]
    const int* __restrict__ row_order, long long nrows, float reg,
    const float* __restrict__ scale, const float* __restrict__ G0) {
    constexpr int K = Geo<KT>::K;
    __shared__ __align__(16) char smem[FP8 ? Geo<KT>::SMEM8 : Geo<KT>::SMEM];
    long long row = blockIdx.x;
    if (row >= nrows) return;
    if (row_order) row = row_order[row];
    const int tid = threadIdx.x;

    const int n = gramian_to_lds<KT, true, false, FP8, WT>(
        smem, indptr, indices, values, factors, row, reg, scale, G0);
    float* A = (float*)smem;
    float* b = A + K * (K + 1);
    if (n == 0) {
        // weighted: an empty sum leaves A = G0 (and b = 0, so x = 0)
        for (int i = tid; i < K * K; i += 256) {
            float a0 = 0.0f;
            if constexpr (WT)
                a0 = G0[max(i / K, i % K) * K + min(i / K, i % K)];
            A_out[row * K * K + i] = a0;
        }
        for (int c = tid; c < K; c += 256) b_out[row * K + c] = 0.0f;
        return;
    }
    for (int i = tid; i < K * K; i += 256)
        A_out[row * K * K + i] = A[(i / K) * (K + 1) + (i % K)];
    for (int c = tid; c < K; c += 256) b_out[row * K + c] = b[c];
}

// Standalone K2: batched SPD solve from dense global A/b.
// phases bitmask (debug/ablation): 1 = eliminate, 2 = solve
template <int KT>
__launch_bounds__(256, 2)
__global__ void k_cholesky_solve(const float* __restrict__ A_in,  // [n][K][K]
                                 const float* __restrict__ b_in,  // [n][K]
                                 float* __restrict__ x_out,       // [n][K]
                                 long long nrows, int phases) {
    constexpr int K = Geo<KT>::K;
    constexpr int NTRI = Geo<KT>::NA;
    __shared__ __align__(16) char smem[Geo<KT>::CHOL_TRI_BYTES];
    const long long row = blockIdx.x;
    if (row >= nrows) return;
    float* A = (float*)smem;
    float* b = A + Geo<KT>::A_TRI_FLOATS;
    const int tid = threadIdx.x;
    {   // load the lower tiles of the (symmetric) square A into the tri
        // image: one whole 16x16 tile per iteration of the 256 threads
        const float* src = A_in + row * (long long)(K * K);
        const int r = tid >> 4, c = tid & 15;
        int I = 0, J = 0;
        for (int t = 0; t < NTRI; ++t) {
            A[t * Geo<KT>::TSZ + r * Geo<KT>::LDT + c] =
                src[(I * 16 + r) * K + J * 16 + c];
            if (++J > I) { ++I; J = 0; }
        }
    }
    for (int c = tid; c < K; c += 256) b[c] = b_in[row * K + c];
    __syncthreads();
    if (phases & 1) cholesky_lds_tri<K>(A);
    if (phases & 2) {
        solve_lds_block_tri<K>(A, b, b + 2 * K, x_out + row * K, nullptr);
    } else if (tid < K) {
        x_out[row * K + tid] = b[tid];
    }
}

// -------- wave-per-entity LDL solver (k <= 64) --------
// The block-per-entity factorization is issue-bound: ~100 instructions of
// work between 2x64 barriers.  For k <= 64 a single wave owns one entity's
// whole [K][K+1] LDS image instead: no barriers (wave-internal LDS ordering
// suffices), 4 independent entities per block, solve fully in registers.
template <int KT>
__launch_bounds__(256)
__global__ void k_ldl_solve_wave(const float* __restrict__ A_in,
                                 const float* __restrict__ b_in,
                                 float* __restrict__ x_out,
                                 unsigned short* __restrict__ x_bf16,
                                 unsigned char* __restrict__ x_fp8,
                                 long long nrows) {
    constexpr int K = KT * 16;
    static_assert(K <= 64, "wave solver handles k <= 64");
    // A lives in LDS as LOWER-TRIANGLE 16x16 tiles only (tile (I,J), I>=J,
    // at triangular offset I(I+1)/2+J).  The LDL never reads above the
    // block diagonal; the panel factorization's upper-scratch trick only
    // needs the diagonal tiles' upper halves, which the full 16x16 tiles
    // keep.  At K=64 this is 10/16 of the square: LDS 66.5 -> 46 KB per
    // block (2 -> 3 waves/SIMD) and 10/16 of the HBM read of A.
    // Tile row stride 18: 8-byte-aligned rows, conflict-free column access
    // (18*i mod 32 distinct over i=0..15).
    constexpr int NP = K / 16;
    constexpr int NTRI = NP * (NP + 1) / 2;
    constexpr int LDT = 18;
    constexpr int TSZ = 16 * LDT;
    __shared__ __align__(16) float As[4][NTRI * TSZ];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + w;
    if (e >= nrows) return;
    float* A = As[w];
    const int li = lane & 15, g4 = lane >> 4;
    {   // load the lower tiles: one whole tile per iteration (16 rows x
        // 4 float4 quads = 64 lanes), contiguous 16-byte global reads
        const float* src = A_in + e * (long long)(K * K);
        const int r = lane >> 2, c4 = lane & 3;
        int I = 0, J = 0;
        for (int t = 0; t < NTRI; ++t) {
            const f32x4 v =
                *(const f32x4*)(src + (I * 16 + r) * K + J * 16 + c4 * 4);
            float* dst = A + t * TSZ + r * LDT + c4 * 4;
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
            if (++J > I) { ++I; J = 0; }
        }
    }
    float x0 = (lane < K) ? b_in[e * K + lane] : 0.0f;
    // In-place LDL^T elimination, 16-column panels with MFMA trailing
    // updates (cdna_hip_programming.md §6 G10: the trailing update
    // A22 -= L21 D^-1 L21^T is matmul-shaped, so it runs on the f32 matrix
    // cores: v_mfma_f32_16x16x4_f32, exact fp32).  Per panel:
    //   (a) factor the panel slab in place, column by column, each lane
    //       updating its own row's panel segment (columns stay raw L*D;
    //       over-length quads CLAMP to the panel edge -- duplicate
    //       same-value writes, never out-of-segment ones);
    //   (b) subtract the panel's outer product from the trailing block as
    //       16x16 MFMA tiles (B operand scaled by -1/D on load).  Tiles on
    //       or above the diagonal write upper-triangle scratch only.
    // Lanes run in wave lockstep, so cross-lane panel dependencies are
    // ordered by program order; no barriers.
    // NOTE: the MFMA tiles need ALL 64 lanes live (every lane carries one
    // (i,k) fragment element regardless of K), so only the row-ownership
    // panel factorization is masked to lane < K; every address in the
    // MFMA phase is bounded by K for all lanes.
    {
        auto tri = [](int I, int J) { return (I * (I + 1)) / 2 + J; };
        // rowseg: lane = global row; its 16-col panel-pi segment lives in
        // tile (lane>>4, pi).  Only dereferenced when P0 <= lane < K.
        for (int pi = 0; pi < NP; ++pi) {
            const int P0 = 16 * pi;
            // (a) panel factorization, fully in registers: each lane holds
            // its row's 16-column panel segment; the pivot column A[c][j]
            // lives in lane c's seg[jj], broadcast by __shfl -- the inner
            // rank-1 update is shfl+fma with ZERO LDS traffic.  Rows above
            // the panel (lane < P0) have no storage in the triangular
            // image and sit the phase out (one exec mask per panel, not
            // per element).
            if (lane >= P0 && lane < K) {
                float* rowseg =
                    A + tri(lane >> 4, pi) * TSZ + (lane & 15) * LDT;
                float seg[16];
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) seg[cc] = rowseg[cc];
#pragma unroll
                for (int jj = 0; jj < 15; ++jj) {
                    const float dj = __shfl(seg[jj], P0 + jj, WAVE);
                    const float dinv = dj > 0.0f ? 1.0f / dj : 0.0f;
                    const float lscl = seg[jj] * dinv;
#pragma unroll
                    for (int cc = jj + 1; cc < 16; ++cc) {
                        const float colj = __shfl(seg[jj], P0 + cc, WAVE);
                        seg[cc] -= lscl * colj;
                    }
                }
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) rowseg[cc] = seg[cc];
            }
            if (pi == NP - 1) break;
            // (b) MFMA trailing update, whole wave.  -1/D per contraction
            // column, local panel col 4*kk + g4.
            const float* Tpp = A + tri(pi, pi) * TSZ;
            float ndk[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int c = 4 * kk + g4;
                const float d = Tpp[c * LDT + c];
                ndk[kk] = d > 0.0f ? -1.0f / d : 0.0f;
            }
            for (int rb = pi + 1; rb < NP; ++rb) {
                const float* TA = A + tri(rb, pi) * TSZ;  // L21 rows rb
                for (int cb = pi + 1; cb <= rb; ++cb) {
                    const float* TB = A + tri(cb, pi) * TSZ;
                    float* TC = A + tri(rb, cb) * TSZ;
                    f32x4 acc;   // C tile: D map row=(l>>4)*4+r, col=l&15
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[r] = TC[(g4 * 4 + r) * LDT + li];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const int pc = 4 * kk + g4;
                        const float a = TA[li * LDT + pc];
                        const float b = TB[li * LDT + pc] * ndk[kk];
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc,
                                                                   0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        TC[(g4 * 4 + r) * LDT + li] = acc[r];
                }
            }
        }
    }
    // solve (I+Ls) y = b ; w = y/D ; (I+Ls^T) x = w, all in registers.
    // Row `lane`'s tiles sit at triangular offsets rowbase + J for J <=
    // lane>>4 (rowbase fixed per lane).
    const int Irow = lane >> 4;
    const float* rowbase = A + ((Irow * (Irow + 1)) / 2) * TSZ + li * LDT;
    const float d0 = (lane < K) ? rowbase[Irow * TSZ + li] : 1.0f;
    const float id0 = d0 > 0.0f ? 1.0f / d0 : 0.0f;
    for (int j = 0; j < K - 1; ++j) {
        const float zj = __shfl(x0, j, WAVE) * __shfl(id0, j, WAVE);
        if (lane > j && lane < K)
            x0 -= rowbase[(j >> 4) * TSZ + (j & 15)] * zj;
    }
    x0 *= id0;
    for (int c = K - 1; c >= 1; --c) {
        const float xc = __shfl(x0, c, WAVE);
        // A(c, lane): row c's tile at column block lane>>4
        if (lane < c)
            x0 -= A[(((c >> 4) * ((c >> 4) + 1)) / 2 + (lane >> 4)) * TSZ
                    + (c & 15) * LDT + li] * id0 * xc;
    }
    if (lane < K) {
        x_out[e * K + lane] = x0;
        if (x_bf16) x_bf16[e * K + lane] = f2bf(x0);
        if (x_fp8) x_fp8[e * K + lane] = f2fp8(x0);
    }
}


// -------- register-resident wave LDL (k <= 64), v2 --------
// A lives in REGISTERS as the 10 lower-triangle 16x16 MFMA C-fragments
// (lane holds (row = (l>>4)*4 + r, col = l&15) of each tile); a 4.35 KB
// per-entity LDS scratch re-shapes one 16-column panel (or one tile
// row/column for the substitution) at a time.  LDS per 4-entity block
// drops 46 -> 17.4 KB and the trailing-update C tiles never touch LDS.
// All tile indices are COMPILE-TIME (constexpr recursion): runtime
// indexing of the fragment array would spill to scratch (guide rule 20).
// Scratch strides: 17 (panel rows, conflict-free columns), 65 (tile-row
// image for the backward substitution).
// WREG_FENCE: the scratch bounces are cross-lane LDS write->read chains
// with no barrier (single wave).  The LDS unit processes a wave's ds ops
// in order, but the COMPILER must not reorder the reads above the masked
// writes (observed miscompile: reader lanes in other row-quads got stale
// panel values) -- a compiler memory fence plus lgkmcnt drain pins the
// order at negligible cost (a handful per entity).
#define WREG_FENCE() __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory")


template <int KT, int PI, int I>
DEV_INLINE void wreg_dump_col(const f32x4* T, float* scr, int g4, int li) {
    if constexpr (I < KT) {
        constexpr int t = tri_off(I, PI);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            scr[((I - PI) * 16 + g4 * 4 + r) * 17 + li] = T[t][r];
        wreg_dump_col<KT, PI, I + 1>(T, scr, g4, li);
    }
}

template <int KT, int PI, int I>
DEV_INLINE void wreg_load_col(f32x4* T, const float* scr, int g4, int li) {
    if constexpr (I < KT) {
        constexpr int t = tri_off(I, PI);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            T[t][r] = scr[((I - PI) * 16 + g4 * 4 + r) * 17 + li];
        wreg_load_col<KT, PI, I + 1>(T, scr, g4, li);
    }
}

template <int KT, int PI, int RB, int CB>
DEV_INLINE void wreg_trail(f32x4* T, const float* scr, const float* ndk,
                           int g4, int li) {
    if constexpr (RB < KT) {
        if constexpr (CB > RB) {
            wreg_trail<KT, PI, RB + 1, PI + 1>(T, scr, ndk, g4, li);
        } else {
            constexpr int t = tri_off(RB, CB);
            f32x4 acc = T[t];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int pc = 4 * kk + g4;
                const float a = scr[((RB - PI) * 16 + li) * 17 + pc];
                const float b =
                    scr[((CB - PI) * 16 + li) * 17 + pc] * ndk[kk];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0,
                                                           0);
            }
            T[t] = acc;
            wreg_trail<KT, PI, RB, CB + 1>(T, scr, ndk, g4, li);
        }
    }
}

// Lane broadcasts of the panel factorization and the substitutions.  Every
// source lane is a compile-time constant, so the broadcast can be a
// v_readlane (VALU -> SGPR, no LDS pipe, no lgkmcnt wait; it ignores EXEC,
// and the source lanes are always live) instead of the ds_bpermute that
// __shfl lowers to.  BC selects how far the broadcasts leave the LDS; the
// arithmetic (operands, order, contraction) is the same at every level,
// so all levels are bit-identical:
//   WREG_BC_SHFL   the __shfl code path, kept as the measured baseline
//   WREG_BC_PANEL  readlane in the panel factorization only
//   WREG_BC_SUBST  + readlane in both substitutions (one broadcast of the
//                  per-lane product x0*id0 in the forward step)
//   WREG_BC_HOIST  + branch-free substitution steps, the block's L entries
//                  read ahead of the serial chain (the default)
// Counters put the kernel at its VALU issue limit at WREG_BC_HOIST (VALU-
// active cycles per SIMD ~ busy cycles, docs/KERNELS.md round 4), so that
// level alone also sheds vector instructions that do not touch a bit:
// packed pairs of panel updates (wreg_update2), keep-or-drop selects under
// literal lane masks instead of per-step compares (wreg_select), and one
// division per pivot shared by the substitutions and the trailing update.
// Levels 0-2 stay the literal baseline the bit-identity tests compare to.
#define WREG_BC_SHFL 0
#define WREG_BC_PANEL 1
#define WREG_BC_SUBST 2
#define WREG_BC_HOIST 3
// L entries read ahead per group in the branch-free substitutions: T[] is
// still live there, so the group is sized to the kernel's 96-VGPR budget
#define WREG_HOIST 8

template <bool RL>
DEV_INLINE float wreg_bcast(float v, int src) {
    if constexpr (RL)
        return __builtin_bit_cast(
            float,
            __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
    else
        return __shfl(v, src, WAVE);
}

// Rounding of the panel's rank-1 updates, pinned.  Written as
// seg[cc] -= lscl * colj the contraction was the compiler's choice: its
// SLP pass paired most of the products across consecutive pivots into
// packed multiplies (then subtracted, two roundings) and fused the rest
// into FMAs -- and it pairs differently once the broadcast operand is a
// scalar register.  The split below is the one every instantiation of the
// shuffle path compiled to (read off the optimized IR), spelled out so
// that all broadcast variants, and later compilers, round identically.
constexpr bool wreg_update_unfused(int jj, int cc) {
    if (jj == 0) return cc >= 2 && cc <= 10 && cc % 2 == 0;
    return cc <= (jj + 10 < 14 ? jj + 10 : 14);
}

DEV_INLINE float wreg_mul_sub(float acc, float a, float b) {
#pragma clang fp contract(off)
    return acc - a * b;
}

// Two neighbouring columns of one pivot step that round the same way
// (wreg_update_unfused() agrees on both) as one packed operation: the
// multiplier lscl is shared, only the broadcast differs.  Per element this
// is exactly wreg_mul_sub() or __builtin_fmaf(-lscl, colj, seg); only the
// instruction count changes (v_pk_mul + v_pk_add, or one v_pk_fma).
typedef float f32x2 __attribute__((ext_vector_type(2)));

DEV_INLINE f32x2 wreg_update2(bool unfused, f32x2 acc, float lscl,
                              f32x2 colj) {
    const f32x2 l = {lscl, lscl};
    if (unfused) {
#pragma clang fp contract(off)
        return acc - l * colj;
    }
    return __builtin_elementwise_fma(-l, colj, acc);
}

// columns (cc, cc+1), cc even, go packed when both round the same way; the
// even alignment keeps one register pair per column pair over all pivots
constexpr bool wreg_update_paired(int jj, int cc) {
    return cc % 2 == 0 && cc > jj && cc + 1 < 16 &&
           wreg_update_unfused(jj, cc) == wreg_update_unfused(jj, cc + 1);
}

// Keep-or-drop select under a lane set that is a compile-time constant:
// the 64-bit mask is a literal in an SGPR pair, no per-step v_cmp.  Lanes
// outside the mask keep `keep` untouched, whatever `take` holds.
DEV_INLINE float wreg_select(unsigned long long mask, float take, float keep) {
    // The mask's high word goes through an opaque 32-bit scalar move.  Left
    // to the compiler, a mask whose high word is all ones (the k = 64 lane
    // sets) becomes one s_mov_b64 with a 32-bit literal, meant sign-extended
    // but encoded (and, on gfx950, executed) as the zero-extended low word:
    // lanes 32..63 dropped out of the select and k = 64 came out wrong.
    unsigned hi = (unsigned)(mask >> 32);
    __asm__("" : "+s"(hi));
    mask = ((unsigned long long)hi << 32) | (unsigned)mask;
    float r;
    __asm__("v_cndmask_b32 %0, %1, %2, %3"
            : "=v"(r) : "v"(keep), "v"(take), "s"(mask));
    return r;
}

constexpr unsigned long long wreg_lanes_below(int n) {   // lanes 0..n-1
    return n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

template <int KT, int PI, int BC>
DEV_INLINE void wreg_panels(f32x4* T, float* scr, int lane, int g4, int li,
                            float& d0) {
    if constexpr (PI < KT) {
        constexpr int K = KT * 16;
        constexpr int P0 = 16 * PI;
        constexpr bool RL = BC >= WREG_BC_PANEL;
        wreg_dump_col<KT, PI, PI>(T, scr, g4, li);
        WREG_FENCE();
        // register factorization of the panel: lane = row P0+lane; lanes
        // 0..15 (always inside the mask) hold the diagonal block
        if (lane < K - P0) {
            float seg[16];
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) seg[cc] = scr[lane * 17 + cc];
#pragma unroll
            for (int jj = 0; jj < 15; ++jj) {
                const float dj = wreg_bcast<RL>(seg[jj], jj);
                const float dinv = dj > 0.0f ? 1.0f / dj : 0.0f;
                const float lscl = seg[jj] * dinv;
#pragma unroll
                for (int cc = jj + 1; cc < 16; ++cc) {
                    if constexpr (BC >= WREG_BC_HOIST) {
                        if (cc % 2 == 1 && wreg_update_paired(jj, cc - 1))
                            continue;          // done with its even partner
                        if (wreg_update_paired(jj, cc)) {
                            const f32x2 colj = {
                                wreg_bcast<true>(seg[jj], cc),
                                wreg_bcast<true>(seg[jj], cc + 1)};
                            const f32x2 s = wreg_update2(
                                wreg_update_unfused(jj, cc),
                                f32x2{seg[cc], seg[cc + 1]}, lscl, colj);
                            seg[cc] = s.x;
                            seg[cc + 1] = s.y;
                            continue;
                        }
                    }
                    const float colj = wreg_bcast<RL>(seg[jj], cc);
                    seg[cc] = wreg_update_unfused(jj, cc)
                                  ? wreg_mul_sub(seg[cc], lscl, colj)
                                  : __builtin_fmaf(-lscl, colj, seg[cc]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) scr[lane * 17 + cc] = seg[cc];
        }
        WREG_FENCE();
        if constexpr (BC >= WREG_BC_HOIST) {
            // The panel's 16 pivots are final: ONE guarded division per
            // pivot serves the substitutions' 1/d (d0 carries the
            // reciprocal itself at this level, see wreg_id0) and, through
            // the scratch's unused pad column (word 16 of the stride-17
            // rows), the trailing update's -1/d.  IEEE division is
            // correctly rounded and rounding is symmetric in sign, so
            // -(1.0f / d) == -1.0f / d bit for bit; the negation is a
            // source modifier of the multiply that consumes it.  Every
            // lane divides (the four lanes of an li write the same word).
            const float d = scr[li * 17 + li];
            const float rinv = d > 0.0f ? 1.0f / d : 0.0f;
            scr[li * 17 + 16] = rinv;
            d0 = wreg_select(0xffffull << P0, rinv, d0);
            wreg_load_col<KT, PI, PI>(T, scr, g4, li);
            if constexpr (PI + 1 < KT) {
                WREG_FENCE();
                float ndk[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    ndk[kk] = -scr[(4 * kk + g4) * 17 + 16];
                wreg_trail<KT, PI, PI + 1, PI + 1>(T, scr, ndk, g4, li);
            }
        } else {
            if (lane >= P0 && lane < P0 + 16)
                d0 = scr[(lane - P0) * 17 + (lane - P0)];
            wreg_load_col<KT, PI, PI>(T, scr, g4, li);
            if constexpr (PI + 1 < KT) {
                float ndk[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int c = 4 * kk + g4;
                    const float d = scr[c * 17 + c];
                    ndk[kk] = d > 0.0f ? -1.0f / d : 0.0f;
                }
                wreg_trail<KT, PI, PI + 1, PI + 1>(T, scr, ndk, g4, li);
            }
        }
        wreg_panels<KT, PI + 1, BC>(T, scr, lane, g4, li, d0);
    }
}

// The substitutions' 1/d from what wreg_panels left in d0: the row's pivot
// (divided here) below WREG_BC_HOIST, the panel's shared reciprocal above.
template <int BC>
DEV_INLINE float wreg_id0(float d0) {
    if constexpr (BC >= WREG_BC_HOIST)
        return d0;
    else
        return d0 > 0.0f ? 1.0f / d0 : 0.0f;
}

template <int KT, int J, int BC>
DEV_INLINE void wreg_forward(const f32x4* T, float* scr, float& x0,
                             float id0, int lane, int g4, int li) {
    if constexpr (J < KT) {
        constexpr int K = KT * 16;
        constexpr int B0 = 16 * J;
        wreg_dump_col<KT, J, J>(T, scr, g4, li);
        WREG_FENCE();
        if constexpr (BC >= WREG_BC_HOIST) {
            // every lane reads a row of the dumped panel (clamped into the
            // rows dump_col wrote) and the step keeps or drops the RESULT:
            // no exec region around the read, so a group's reads issue
            // ahead of the chain.  Selecting the result, not the L entry,
            // keeps idle lanes untouched whatever the broadcast value is
            // (a zeroed L entry would still flip a -0.0 or spread a NaN).
            const int lrow = (lane < K ? lane : K - 1) - B0;
            const float* lp = scr + (lrow > 0 ? lrow : 0) * 17;
            constexpr int NS = (K - 1 - B0 < 16) ? K - 1 - B0 : 16;
#pragma unroll
            for (int t0 = 0; t0 < NS; t0 += WREG_HOIST) {
                float l[WREG_HOIST];
#pragma unroll
                for (int u = 0; u < WREG_HOIST; ++u)
                    if (t0 + u < NS) l[u] = lp[t0 + u];
#pragma unroll
                for (int u = 0; u < WREG_HOIST; ++u) {
                    if (t0 + u < NS) {
                        const int j = B0 + t0 + u;
                        const float zj = wreg_bcast<true>(x0 * id0, j);
                        const float xn = __builtin_fmaf(-l[u], zj, x0);
                        // lanes j+1 .. K-1
                        x0 = wreg_select(wreg_lanes_below(K) &
                                             ~wreg_lanes_below(j + 1),
                                         xn, x0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int j = B0 + t;
                if (j >= K - 1) break;
                float zj;
                if constexpr (BC >= WREG_BC_SUBST)
                    zj = wreg_bcast<true>(x0 * id0, j);
                else
                    zj = __shfl(x0, j, WAVE) * __shfl(id0, j, WAVE);
                if (lane > j && lane < K)
                    x0 = __builtin_fmaf(-scr[(lane - B0) * 17 + t], zj, x0);
            }
        }
        wreg_forward<KT, J + 1, BC>(T, scr, x0, id0, lane, g4, li);
    }
}

template <int KT, int I, int J>
DEV_INLINE void wreg_dump_row(const f32x4* T, float* scr, int g4, int li) {
    if constexpr (J <= I) {
        constexpr int t = tri_off(I, J);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            scr[(g4 * 4 + r) * 65 + J * 16 + li] = T[t][r];
        wreg_dump_row<KT, I, J + 1>(T, scr, g4, li);
    }
}

template <int KT, int I, int BC>
DEV_INLINE void wreg_backward(const f32x4* T, float* scr, float& x0,
                              float id0, int lane, int g4, int li) {
    if constexpr (I >= 0) {
        constexpr int B0 = 16 * I;
        wreg_dump_row<KT, I, 0>(T, scr, g4, li);
        WREG_FENCE();
        if constexpr (BC >= WREG_BC_HOIST) {
            // t*65 + lane <= 15*65 + 63 stays inside the 1040-float
            // scratch for every lane; lanes >= c read stale words that
            // the result select drops
            constexpr int T0 = (I == 0) ? 1 : 0;    // c = B0 + t >= 1
#pragma unroll
            for (int t1 = 16; t1 > T0; t1 -= WREG_HOIST) {
                float m[WREG_HOIST];
#pragma unroll
                for (int u = 0; u < WREG_HOIST; ++u)
                    if (t1 - 1 - u >= T0)
                        m[u] = scr[(t1 - 1 - u) * 65 + lane] * id0;
#pragma unroll
                for (int u = 0; u < WREG_HOIST; ++u) {
                    if (t1 - 1 - u >= T0) {
                        const int c = B0 + t1 - 1 - u;
                        const float xc = wreg_bcast<true>(x0, c);
                        const float xn = __builtin_fmaf(-m[u], xc, x0);
                        x0 = wreg_select(wreg_lanes_below(c), xn, x0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 15; t >= 0; --t) {
                const int c = B0 + t;
                if (c < 1) break;
                const float xc =
                    wreg_bcast<(BC >= WREG_BC_SUBST)>(x0, c);
                if (lane < c)
                    x0 = __builtin_fmaf(-(scr[t * 65 + lane] * id0), xc, x0);
            }
        }
        wreg_backward<KT, I - 1, BC>(T, scr, x0, id0, lane, g4, li);
    }
}

// What the register-LDL kernels store for a NaN result: the canonical quiet
// NaN.  Sign and payload of a NaN say nothing about the system, and they
// are not the source's to decide: they follow where the compiler puts a
// negation (on a multiply's operand, on an FMA's, or into the reciprocal's
// select) and in which order it hands two NaN operands to an instruction,
// and it chooses differently at each broadcast level.  On integer bits, so
// that no floating-point fold can see through it.
DEV_INLINE float wreg_canon_nan(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return __builtin_bit_cast(float,
                              (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u
                                                              : u);
}

template <int KT, int t>
DEV_INLINE void wreg_load_A(f32x4* T, const float* src, int g4, int li) {
    if constexpr (t < KT * (KT + 1) / 2) {
        constexpr int K = KT * 16;
        constexpr int I = lo_tile_i(t);
        constexpr int J = t - (I * (I + 1)) / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            T[t][r] = src[(I * 16 + g4 * 4 + r) * K + J * 16 + li];
        wreg_load_A<KT, t + 1>(T, src, g4, li);
    }
}

template <int KT, int BC>
__launch_bounds__(256)
// the lean variant sits at 75 VGPRs; left alone the allocator adds 24 AGPRs
// on top and lands one register granule past 5 waves per SIMD
__attribute__((amdgpu_waves_per_eu(BC >= WREG_BC_HOIST ? 5 : 1)))
__global__ void k_ldl_solve_wave_reg(const float* __restrict__ A_in,
                                     const float* __restrict__ b_in,
                                     float* __restrict__ x_out,
                                     unsigned short* __restrict__ x_bf16,
                                     unsigned char* __restrict__ x_fp8,
                                     long long nrows) {
    constexpr int K = KT * 16;
    static_assert(K <= 64, "register wave solver handles k <= 64");
    constexpr int NTRI = KT * (KT + 1) / 2;
    constexpr int SCR = K * 17;            // covers 16*65=1040 too (K=64)
    __shared__ __align__(16) float As[4][SCR > 1040 ? SCR : 1040];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + w;
    if (e >= nrows) return;
    float* scr = As[w];
    const int li = lane & 15, g4 = lane >> 4;

    f32x4 T[NTRI];
    wreg_load_A<KT, 0>(T, A_in + e * (long long)(K * K), g4, li);
    float x0 = (lane < K) ? b_in[e * K + lane] : 0.0f;
    float d0 = 1.0f;
    wreg_panels<KT, 0, BC>(T, scr, lane, g4, li, d0);
    const float id0 = wreg_id0<BC>(d0);
    wreg_forward<KT, 0, BC>(T, scr, x0, id0, lane, g4, li);
    x0 *= id0;
    wreg_backward<KT, KT - 1, BC>(T, scr, x0, id0, lane, g4, li);
    x0 = wreg_canon_nan(x0);
    if (lane < K) {
        x_out[e * K + lane] = x0;
        if (x_bf16) x_bf16[e * K + lane] = f2bf(x0);
        if (x_fp8) x_fp8[e * K + lane] = f2fp8(x0);
    }
}

// -------- wave-fused ALS solve (k <= 64): Gramian + LDL in ONE wave --------
// r2 profiling: with the v2 multi-chunk gramian the modular path became
// A-round-trip bound — the gramian writes nrows*K*K fp32 to HBM (~2.9 TB/s)
// and the wave solver reads the lower tiles back (~1.5 TB/s).  This kernel
// removes that traffic entirely: one WAVE owns one entity end to end and
// the Gramian MFMAs accumulate DIRECTLY into the lower-triangle C-fragment
// tiles T[] that the register LDL (wreg_panels/forward/backward) consumes.
// No barriers anywhere (wave-local LDS + WREG_FENCE ordering); gather
// stalls of one wave overlap solver compute of the others.
//
// Tile algebra: lower tile (I,J) = mfma(frag[I], frag[J]) — D[row][col] =
// sum_r G[r][I*16+row]*G[r][J*16+col] = A[I*16+row][J*16+col], exactly the
// (g4*4+r, li) layout wreg_load_A produced in the modular path.  b comes
// from KT EXT tiles (cols 0/1 = rating hi/lo), redistributed to
// x0 = b[lane] through a 128-float LDS bounce.

template <int KT, bool FP8, int t = 0>
DEV_INLINE void mfma_lower_tiles(const typename FragT<FP8>::type* frag,
                                 f32x4* T) {
    if constexpr (t < KT * (KT + 1) / 2) {
        constexpr int I = lo_tile_i(t);
        constexpr int J = t - (I * (I + 1)) / 2;
        if constexpr (FP8)
            T[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                frag[I], frag[J], T[t], 0, 0, 0);
        else
            T[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                frag[I], frag[J], T[t], 0, 0, 0);
        mfma_lower_tiles<KT, FP8, t + 1>(frag, T);
    }
}

template <int KT, bool FP8, int P = 0>
DEV_INLINE void mfma_ext_tiles(const typename FragT<FP8>::type* frag,
                               f32x4* E) {
    if constexpr (P < KT) {
        if constexpr (FP8)
            E[P] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                frag[P], frag[KT], E[P], 0, 0, 0);
        else
            E[P] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                frag[P], frag[KT], E[P], 0, 0, 0);
        mfma_ext_tiles<KT, FP8, P + 1>(frag, E);
    }
}

template <int KT, int P = 0>
DEV_INLINE void wavefused_dump_b(const f32x4* E, float* scr, int g4, int li) {
    if constexpr (P < KT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (li == 0) scr[P * 16 + g4 * 4 + r] = E[P][r];
            else if (li == 1) scr[64 + P * 16 + g4 * 4 + r] = E[P][r];
        }
        wavefused_dump_b<KT, P + 1>(E, scr, g4, li);
    }
}

// Rounding of diag + reg*n, pinned like the panel updates above.  Written
// as T + regn the contraction is the compiler's choice, and it chose by
// basic block: every instantiation of the branching form below fuses the
// product into the add (one rounding) except, at k = 64, for the diagonal
// tiles past the first, whose adds sink behind the first panel and take
// the rounded product (read off the ISA of every instantiation).  The
// branch-free form would be fused everywhere, so it spells the split out.
constexpr bool wavefused_diag_unfused(int KT, int I) {
    return KT == 4 && I >= 1;
}

DEV_INLINE float wreg_mul_add(float acc, float a, float b) {
#pragma clang fp contract(off)
    return acc + a * b;
}

template <int KT, int BC, int I = 0>
DEV_INLINE void wavefused_diag(f32x4* T, float reg, float nf, int g4,
                               int li) {
    if constexpr (I < KT) {
        constexpr int t = tri_off(I, I);
        const float regn = reg * nf;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (BC >= WREG_BC_HOIST) {
                // li == g4*4 + r holds on lanes 20*g4 + r: a constant set
                const float dd = wavefused_diag_unfused(KT, I)
                                     ? wreg_mul_add(T[t][r], reg, nf)
                                     : __builtin_fmaf(reg, nf, T[t][r]);
                T[t][r] = wreg_select(0x1000010000100001ull << r,
                                      dd <= 0.0f ? 1.0f : dd, T[t][r]);
            } else if (li == g4 * 4 + r) {
                const float dd = T[t][r] + regn;
                T[t][r] = dd <= 0.0f ? 1.0f : dd;   // degenerate guard
            }
        }
        wavefused_diag<KT, BC, I + 1>(T, reg, nf, g4, li);
    }
}

// Split staging for the double-buffered wave-fused variant: issue the
// gathers for chunk ch+1 (registers only, no wait) BEFORE chunk ch's
// MFMAs, commit the transpose+LDS writes after — the load latency hides
// behind the matrix work instead of stalling the wave.
template <int KT, bool FP8>
struct StagedRegs {
    uint4 v[4];
    unsigned ext_h, ext_l;
};

template <int KT, bool FP8>
DEV_INLINE void stage_loads(StagedRegs<KT, FP8>& sr,
                            const int* __restrict__ indices,
                            const float* __restrict__ values,
                            const void* __restrict__ factors_v,
                            long long base, int nrem, int lane) {
    constexpr int K = Geo<KT>::K;
    static_assert(FP8, "double-buffer staging: fp8 path only");
    const unsigned char* factors = (const unsigned char*)factors_v;
    constexpr int NT = 8 * (K / 16);
    if (lane < NT) {
        const int q = lane & 7, c16 = lane >> 3;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint4 x = {0, 0, 0, 0};
            const int row = 4 * q + m;
            if (row < nrem) {
                const long long col = indices[base + row];
                x = *(const uint4*)(factors + col * (long long)K + c16 * 16);
            }
            sr.v[m] = x;
        }
    }
    if (lane < 8) {
        unsigned h = 0, l = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = 4 * lane + m;
            const float r = (row < nrem) ? values[base + row] : 0.0f;
            const unsigned char hb = f2fp8(r);
            const unsigned char lb = f2fp8(r - fp82f(hb));
            h |= ((unsigned)hb) << (8 * m);
            l |= ((unsigned)lb) << (8 * m);
        }
        sr.ext_h = h;
        sr.ext_l = l;
    }
}

template <int KT, bool FP8>
DEV_INLINE void stage_commit(const StagedRegs<KT, FP8>& sr, char* buf,
                             int lane) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = Geo<KT>::TROW8;
    constexpr int NT = 8 * (K / 16);
    if (lane < NT) {
        const int q = lane & 7, c16 = lane >> 3;
        char* rb = buf + (long long)(16 * c16) * TROW + q * 4;
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
            unsigned wd = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                wd |= (((&sr.v[m].x)[cc >> 2] >> (8 * (cc & 3))) & 0xffu)
                      << (8 * m);
            *(unsigned*)(rb + (long long)cc * TROW) = wd;
        }
    }
    if (lane < 8) {
        *(unsigned*)(buf + (long long)K * TROW + lane * 4) = sr.ext_h;
        *(unsigned*)(buf + (long long)(K + 1) * TROW + lane * 4) = sr.ext_l;
    }
}

// Double-buffered wave-fused ALS solve (fp8, k <= 64): same math as
// k_als_solve_wavefused, software-pipelined staging.
template <int KT, int BC>
__launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(4)))
__global__ void k_als_solve_wavefused_db(const long long* __restrict__ indptr,
                                         const int* __restrict__ indices,
                                         const float* __restrict__ values,
                                         const void* __restrict__ factors,
                                         float* __restrict__ out_f32,
                                         unsigned short* __restrict__ out_bf16,
                                         unsigned char* __restrict__ out_fp8,
                                         const int* __restrict__ row_order,
                                         long long nrows, float reg) {
    constexpr int K = KT * 16;
    static_assert(K <= 64, "wave-fused path handles k <= 64");
    constexpr int NA = KT * (KT + 1) / 2;
    constexpr int TROW = Geo<KT>::TROW8;
    constexpr int SB = (K + 16) * TROW;
    constexpr int SCRF = (K * 17 > 1040) ? K * 17 : 1040;
    constexpr int WB0 = (2 * SB > SCRF * 4) ? 2 * SB : SCRF * 4;
    constexpr int WB = (WB0 + 15) & ~15;
    __shared__ __align__(16) char smem[4 * WB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long e0 = (long long)blockIdx.x * 4 + w;
    if (e0 >= nrows) return;
    const long long e = row_order ? row_order[e0] : e0;
    char* base = smem + (long long)w * WB;
    float* scr = (float*)base;
    const int g4 = lane >> 4, li = lane & 15;
    const long long p0 = indptr[e];
    const int n = (int)(indptr[e + 1] - p0);
    if (n == 0) {
        if (lane < K) {
            out_f32[e * K + lane] = 0.0f;
            if (out_bf16) out_bf16[e * K + lane] = 0;
            if (out_fp8) out_fp8[e * K + lane] = 0;
        }
        return;
    }
    for (int b = 0; b < 2; ++b)
        for (int i = lane; i < 14 * 8; i += WAVE) {
            const int row = K + 2 + i / 8, seg = i % 8;
            *(unsigned*)(base + b * SB + (long long)row * TROW + seg * 4) =
                0u;
        }
    f32x4 T[NA], E[KT];
#pragma unroll
    for (int t = 0; t < NA; ++t) T[t] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < KT; ++p) E[p] = f32x4{0, 0, 0, 0};
    const int nchunks = (n + 31) >> 5;
    StagedRegs<KT, true> sr;
    stage_loads<KT, true>(sr, indices, values, factors, p0, n, lane);
    stage_commit<KT, true>(sr, base, lane);
#pragma unroll 1
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks)
            stage_loads<KT, true>(sr, indices, values, factors,
                                  p0 + (long long)(ch + 1) * 32,
                                  n - (ch + 1) * 32, lane);
        WREG_FENCE();
        typename FragT<true>::type frag[KT + 1];
        read_frags<KT, true>(base + (ch & 1) * SB, lane, frag);
        WREG_FENCE();
        mfma_lower_tiles<KT, true>(frag, T);
        mfma_ext_tiles<KT, true>(frag, E);
        if (ch + 1 < nchunks)
            stage_commit<KT, true>(sr, base + ((ch + 1) & 1) * SB, lane);
    }
    wavefused_dump_b<KT>(E, scr, g4, li);
    WREG_FENCE();
    float x0 = (lane < K) ? scr[lane] + scr[64 + lane] : 0.0f;
    WREG_FENCE();
    wavefused_diag<KT, BC>(T, reg, (float)n, g4, li);
    float d0 = 1.0f;
    wreg_panels<KT, 0, BC>(T, scr, lane, g4, li, d0);
    const float id0 = wreg_id0<BC>(d0);
    wreg_forward<KT, 0, BC>(T, scr, x0, id0, lane, g4, li);
    x0 *= id0;
    wreg_backward<KT, KT - 1, BC>(T, scr, x0, id0, lane, g4, li);
    x0 = wreg_canon_nan(x0);
    if (lane < K) {
        out_f32[e * K + lane] = x0;
        if (out_bf16) out_bf16[e * K + lane] = f2bf(x0);
        if (out_fp8) out_fp8[e * K + lane] = f2fp8(x0);
    }
}

// T[] = the lower tiles of the symmetric base matrix G0 ([K][K] fp32), in
// the C-fragment layout the LDL consumes (row 16I + 4*g4 + r, column
// 16J + li): wreg_load_A's map, with the diagonal tiles reading
// G0[max][min] so that nothing above the diagonal is touched.
template <int KT, int t = 0>
DEV_INLINE void wavefused_load_base(f32x4* T, const float* __restrict__ G0,
                                    int g4, int li) {
    if constexpr (t < KT * (KT + 1) / 2) {
        constexpr int K = KT * 16;
        constexpr int I = lo_tile_i(t);
        constexpr int J = t - (I * (I + 1)) / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I * 16 + g4 * 4 + r, col = J * 16 + li;
            if constexpr (I == J)
                T[t][r] = G0[max(row, col) * K + min(row, col)];
            else
                T[t][r] = G0[row * K + col];
        }
        wavefused_load_base<KT, t + 1>(T, G0, g4, li);
    }
}

template <int KT, bool FP8, int BC, bool WT = false>
__launch_bounds__(256)
// waves_per_eu(5): 96 VGPRs with ~12-17 spilled (52-60 B/lane scratch) buys
// a 5th wave/SIMD over the natural 105-reg allocation — measured 3.23 ->
// 2.65 ms/iter on the rank-64 headline (the spill traffic hides behind the
// same gather stalls the extra wave fills).  With the readlane broadcasts
// (BC >= WREG_BC_PANEL) the panel's operands sit in SGPRs and the same cap
// is met at 95 VGPRs with no spill at all.
__attribute__((amdgpu_waves_per_eu(5)))
__global__ void k_als_solve_wavefused(const long long* __restrict__ indptr,
                                      const int* __restrict__ indices,
                                      const float* __restrict__ values,
                                      const void* __restrict__ factors,
                                      float* __restrict__ out_f32,
                                      unsigned short* __restrict__ out_bf16,
                                      unsigned char* __restrict__ out_fp8,
                                      const int* __restrict__ row_order,
                                      long long nrows, float reg,
                                      const float* __restrict__ scale,
                                      const float* __restrict__ G0) {
    constexpr int K = KT * 16;
    static_assert(K <= 64, "wave-fused path handles k <= 64");
    constexpr int NA = KT * (KT + 1) / 2;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    constexpr int SB = (K + 16) * TROW;            // stage bytes per wave
    // split-wave staging: a chunk's gather tasks only need NT lanes (fp8
    // K=64: 32); when two chunks' tasks fit in one wave, the upper half
    // stages chunk ch+1 into a second buffer in the SAME instructions —
    // double the gathers in flight at zero extra registers or occupancy
    constexpr int NT = FP8 ? 8 * (K / 16) : K;
    constexpr int NCHW = (2 * NT <= WAVE && NT >= 8) ? 2 : 1;
    constexpr int SCRF = (K * 17 > 1040) ? K * 17 : 1040;  // solver scratch
    constexpr int WB0 = (NCHW * SB > SCRF * 4) ? NCHW * SB : SCRF * 4;
    constexpr int WB = (WB0 + 15) & ~15;
    __shared__ __align__(16) char smem[4 * WB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long e0 = (long long)blockIdx.x * 4 + w;
    if (e0 >= nrows) return;
    const long long e = row_order ? row_order[e0] : e0;
    char* buf = smem + (long long)w * WB;
    float* scr = (float*)buf;          // union: stage dies before the solve
    const int g4 = lane >> 4, li = lane & 15;
    const long long p0 = indptr[e];
    const int n = (int)(indptr[e + 1] - p0);
    if (n == 0) {
        if (lane < K) {
            out_f32[e * K + lane] = 0.0f;
            if (out_bf16) out_bf16[e * K + lane] = 0;
            if (out_fp8) out_fp8[e * K + lane] = 0;
        }
        return;
    }
    // zero the EXT pad rows K+2..K+15 of my NCHW buffers (wave-local)
#pragma unroll
    for (int b = 0; b < NCHW; ++b)
        stage_zero_pad<KT, FP8>(buf + b * SB, lane, WAVE);
    f32x4 T[NA], E[KT];
    if constexpr (WT) {
        wavefused_load_base<KT>(T, G0, g4, li);
    } else {
#pragma unroll
        for (int t = 0; t < NA; ++t) T[t] = f32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int p = 0; p < KT; ++p) E[p] = f32x4{0, 0, 0, 0};
    const int nchunks = (n + 31) >> 5;
    for (int ch = 0; ch < nchunks; ch += NCHW) {
        if constexpr (NCHW == 2) {
            // Everything is counted from the pair's first rating, cb, with
            // rem ratings left: both wave-uniform.  A full trip (all 64
            // ratings present) is the common case and takes the unguarded
            // staging, see stage_gather4.  When chunk ch+1 does not exist
            // its rows all lie past rem and stage as zeros into the second
            // buffer, which is then not read.
            const int rem = n - ch * 32;
            const bool full = rem >= 64;
            const long long cb = p0 + (long long)ch * 32;
            // the EXT rows have a lane map of their own: lanes 0-31 own
            // the ratings of chunk ch, lanes 32-63 those of chunk ch+1,
            // so lane l owns rating l of the pair
            const float xr = stage_ext_load(values, cb, rem, lane, full);
            const int sub = (lane >= NT) ? 1 : 0;
            if (2 * NT == WAVE || lane < 2 * NT)
                stage_gather_w<KT, FP8, NT, WT>(buf + sub * SB, indices,
                                                factors, cb, rem,
                                                lane - sub * NT, 32 * sub,
                                                full, scale);
            stage_ext_commit<KT, FP8>(buf + (lane >> 5) * SB, lane & 31, xr);
        } else {
            stage_chunk_w<KT, FP8, WAVE, WT>(buf, indices, values, factors,
                                             p0 + (long long)ch * 32,
                                             n - ch * 32, lane, scale);
        }
        WREG_FENCE();                  // cross-lane LDS write -> read
        {
            typename FragT<FP8>::type frag[KT + 1];
            read_frags<KT, FP8>(buf, lane, frag);
            mfma_lower_tiles<KT, FP8>(frag, T);
            mfma_ext_tiles<KT, FP8>(frag, E);
        }
        if constexpr (NCHW == 2) {
            if (ch + 1 < nchunks) {
                typename FragT<FP8>::type frag[KT + 1];
                read_frags<KT, FP8>(buf + SB, lane, frag);
                mfma_lower_tiles<KT, FP8>(frag, T);
                mfma_ext_tiles<KT, FP8>(frag, E);
            }
        }
        WREG_FENCE();                  // reads drained before next stage
    }
    // b = bhi + blo redistributed to lane = row; then lambda*n*I
    wavefused_dump_b<KT>(E, scr, g4, li);
    WREG_FENCE();
    float x0 = (lane < K) ? scr[lane] + scr[64 + lane] : 0.0f;
    WREG_FENCE();                      // b read before panel dumps reuse scr
    wavefused_diag<KT, BC>(T, reg, (float)n, g4, li);
    // in-register LDL + substitution (shared with k_ldl_solve_wave_reg)
    float d0 = 1.0f;
    wreg_panels<KT, 0, BC>(T, scr, lane, g4, li, d0);
    const float id0 = wreg_id0<BC>(d0);
    wreg_forward<KT, 0, BC>(T, scr, x0, id0, lane, g4, li);
    x0 *= id0;
    wreg_backward<KT, KT - 1, BC>(T, scr, x0, id0, lane, g4, li);
    x0 = wreg_canon_nan(x0);
    if (lane < K) {
        out_f32[e * K + lane] = x0;
        if (out_bf16) out_bf16[e * K + lane] = f2bf(x0);
        if (out_fp8) out_fp8[e * K + lane] = f2fp8(x0);
    }
}

// -------- factor Gram matrix G = F^T F (the implicit-feedback base) --------
// F: a bf16 / e4m3 factor table [n][K].  One WAVE owns one part of
// rows_per_part (a multiple of 32) consecutive rows: each 32-row chunk goes
// through the transposed stage (stage_chunk_w<IDENT>) and the lower-tile
// MFMAs of the wave-fused kernel, and the wave's partial lower tiles land
// in ws[part][K][K].  k_factor_gram_reduce then sums the parts in part
// order and mirrors the lower triangle: no floating-point atomics, so G is
// bit-reproducible, and exactly symmetric.  Rows >= n stage as zeros.
// An e4m3 table is widened to bf16 while staging (exact: every e4m3 value
// is a bf16 value) and contracted by the bf16 MFMA: the fp8 MFMA sums its
// 32 products with ~2^-17 relative precision (measured, docs/KERNELS.md),
// short of the fp32 dot bound this matrix is held to -- it is added to
// EVERY entity's normal equations.
//
// ROWS: G = sum_j F[rows[j]] F[rows[j]]^T over a row list (the live item
// rows of a serving table).  n is the list length; parts, chunks and the
// reduction run over list positions exactly as above, only the address of
// a staged row changes (the guarded gather of stage_gather_w, no EXT rows).
// Positions >= n stage as zeros and neither read rows[] nor load from the
// table.  Rows may repeat (a repeated row counts once per occurrence) and
// come in any order; every entry must be a row of the table -- the caller
// checks, the kernel does not.  With the same rows_per_part the result is
// bit-equal to the plain kernel on the compacted table F[rows]: it is the
// same MFMA sequence, hence as reproducible and as symmetric.
template <int KT, int t = 0>
DEV_INLINE void factor_gram_store(const f32x4* T, float* dst, int g4, int li) {
    if constexpr (t < KT * (KT + 1) / 2) {
        constexpr int K = KT * 16;
        constexpr int I = lo_tile_i(t);
        constexpr int J = t - (I * (I + 1)) / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            dst[(I * 16 + g4 * 4 + r) * K + J * 16 + li] = T[t][r];
        factor_gram_store<KT, t + 1>(T, dst, g4, li);
    }
}

template <int KT, bool FP8, bool ROWS = false>
__launch_bounds__(256)
__global__ void k_factor_gram(
    const typename GatherT<FP8>::elem* __restrict__ factors,
    const int* __restrict__ rows,  // ROWS: [n] table rows, else unused
    float* __restrict__ ws,      // [parts][K][K], lower tiles written
    long long n, long long rows_per_part, long long parts) {
    constexpr int K = KT * 16;
    constexpr int NA = KT * (KT + 1) / 2;
    constexpr int TROW = Geo<KT>::TROW;            // bf16 stage either way
    constexpr int SB = ((K + 16) * TROW + 15) & ~15;
    constexpr int FB = 16;
    __shared__ __align__(16) char smem[4 * SB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long part = (long long)blockIdx.x * 4 + w;
    if (part >= parts) return;
    char* buf = smem + (long long)w * SB;
    const int g4 = lane >> 4, li = lane & 15;
    f32x4 T[NA];
#pragma unroll
    for (int t = 0; t < NA; ++t) T[t] = f32x4{0, 0, 0, 0};
    const long long r0 = part * rows_per_part;
    const long long r1 = min(n, r0 + rows_per_part);
    for (long long base = r0; base < r1; base += 32) {
        const int nrem = (int)min((long long)32, r1 - base);
        if constexpr (ROWS)
            stage_gather_w<KT, false, WAVE, false, false, FP8>(
                buf, rows, factors, base, nrem, lane, 0, false);
        else
            stage_chunk_w<KT, false, WAVE, false, true, FP8>(
                buf, nullptr, nullptr, factors, base, nrem, lane);
        WREG_FENCE();                  // cross-lane LDS write -> read
        bf16x8 frag[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t)
            frag[t] = *(const bf16x8*)(
                buf + (long long)(t * 16 + li) * TROW + g4 * FB);
        mfma_lower_tiles<KT, false>(frag, T);
        WREG_FENCE();                  // reads drained before next stage
    }
    factor_gram_store<KT>(T, ws + part * (long long)(K * K), g4, li);
}

template <int KT>
__launch_bounds__(256)
__global__ void k_factor_gram_reduce(const float* __restrict__ ws,
                                     float* __restrict__ G, long long parts) {
    constexpr int K = KT * 16;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * K) return;
    const int i = idx / K, j = idx % K;
    if (i < j) return;                 // (i, j) is written from (j, i)
    float acc = 0.0f;
    for (long long p = 0; p < parts; ++p) acc += ws[p * (K * K) + idx];
    G[i * K + j] = acc;
    G[j * K + i] = acc;
}

// ------------------------------------------------------------- MFMA probes
// Layout-validation kernels for tests/test_gpu_mfma.py.

// f32 16x16x4 probe with the guide-documented operand maps
// (cdna_hip_programming.md §3): definitive C/D-layout check.
__global__ void k_mfma_probe_f32(const float* __restrict__ Amat,  // [16][4]
                                 const float* __restrict__ Bmat,  // [4][16]
                                 float* __restrict__ D) {         // [16][16]
    const int lane = threadIdx.x;
    const float a = Amat[(lane & 15) * 4 + (lane >> 4)];
    const float b = Bmat[(lane >> 4) * 16 + (lane & 15)];
    f32x4 acc{0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        D[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

// bf16 16x16x32 probe through the exact stage/frag machinery of the Gramian:
// C[16][16] = Xt^T @ Yt for Xt, Yt [32][16] bf16.
__global__ void k_mfma_probe_bf16(const unsigned short* __restrict__ Xt,
                                  const unsigned short* __restrict__ Yt,
                                  float* __restrict__ C) {
    auto stage_xor = [](int row) -> unsigned { return (row & 8) ? 32u : 0u; };
    constexpr int SP = 32;  // 2 tiles of 16 cols; SP*2 = 64B, XOR-closed
    __shared__ __align__(16) unsigned short st[32 * SP];
    const int lane = threadIdx.x;  // launched with 64 threads
    {
        const int row = lane & 31, tile = lane >> 5;
        const unsigned short* src = (tile == 0 ? Xt : Yt) + row * 16;
        for (int h = 0; h < 2; ++h) {
            unsigned byte = (unsigned)(row * SP + tile * 16 + h * 8) * 2u
                            ^ stage_xor(row);
            *(uint4*)((char*)st + byte) = *(const uint4*)(src + h * 8);
        }
    }
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
    const unsigned xorb = (g & 1) ? 32u : 0u;
    bf16x8 frag[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            unsigned byte = (unsigned)((8 * g + j) * SP + t * 16 + li) * 2u;
            f[j] = *(const short*)((const char*)st + (byte ^ xorb));
        }
        frag[t] = f;
    }
    f32x4 acc{0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag[0], frag[1], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        C[(g * 4 + r) * 16 + li] = acc[r];
}

// fp8 e4m3 16x16x32 probe through the fp8 stage geometry (TROW8 rows,
// ds_read_b64 fragments): C[16][16] = Xt^T @ Yt for Xt, Yt [32][16] e4m3
// bytes.  Validates the (lane, element) map + C/D layout assumption of
// k_gramian<KT, true> against a torch reference (tests/test_gpu_mfma.py).
__global__ void k_mfma_probe_fp8(const unsigned char* __restrict__ Xt,
                                 const unsigned char* __restrict__ Yt,
                                 float* __restrict__ C) {
    constexpr int TROW8 = 40;
    __shared__ __align__(8) char st[32 * TROW8];
    const int lane = threadIdx.x;  // launched with 64 threads
    for (int i = lane; i < 2 * 16 * 32; i += 64) {
        const int tile = i >> 9, rem = i & 511;
        const int r = rem >> 4, c = rem & 15;   // rating r, column c
        st[(tile * 16 + c) * TROW8 + r] = (tile == 0 ? Xt : Yt)[r * 16 + c];
    }
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
    const fp8x8 fx = *(const fp8x8*)(st + (li)*TROW8 + g * 8);
    const fp8x8 fy = *(const fp8x8*)(st + (16 + li) * TROW8 + g * 8);
    f32x4 acc{0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(fx, fy, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        C[(g * 4 + r) * 16 + li] = acc[r];
}

// -------------------------------------------------------------- launchers
// The definitions of fma_api.h's ALS entry points.  Each checks k and
// nrows, picks the instantiation through dispatch_ic (k/16, then the gather
// precision or the broadcast variant where the kernel has one) and returns
// the launch status.

namespace {

const dim3 kBlock(256);
// one entity per block / four entities (one per wave) per block
inline dim3 grid_block(long long nrows) { return dim3((unsigned)nrows); }
inline dim3 grid_wave(long long nrows) {
    return dim3((unsigned)((nrows + 3) / 4));
}
inline bool bad_shape(int k, long long nrows) {
    return k % 16 != 0 || nrows <= 0;
}

}  // namespace

extern "C" const char* fma_err_str(int err) {
    return hipGetErrorString((hipError_t)err);
}

// WT = false: the explicit kernels (scale / base null); WT = true: the
// weighted twins, ``values`` carrying ext[]
template <bool WT>
static int launch_als_solve_fused(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* values, const void* factors, float* out_f32,
    unsigned short* out_bf16, unsigned char* out_fp8, const int* row_order,
    long long nrows, float reg, const float* scale, const float* base,
    void* stream) {
    if (bad_shape(k, nrows) || (fp8 ? out_bf16 != nullptr : out_fp8 != nullptr))
        return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4, 5, 6, 7, 8>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (fp8)
            k_als_solve_fused<KT, true, WT>
                <<<grid_block(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, values, (const unsigned char*)factors,
                    out_f32, out_fp8, row_order, nrows, reg, scale, base);
        else
            k_als_solve_fused<KT, false, WT>
                <<<grid_block(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, values, (const unsigned short*)factors,
                    out_f32, out_bf16, row_order, nrows, reg, scale, base);
        return hipGetLastError();
    });
}

extern "C" int fma_als_solve_fused(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* values, const void* factors, float* out_f32,
    unsigned short* out_bf16, unsigned char* out_fp8, const int* row_order,
    long long nrows, float reg, void* stream) {
    return launch_als_solve_fused<false>(
        k, fp8, indptr, indices, values, factors, out_f32, out_bf16, out_fp8,
        row_order, nrows, reg, nullptr, nullptr, stream);
}

extern "C" int fma_als_solve_fused_w(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* scale, const float* ext, const float* base,
    const void* factors, float* out_f32, unsigned short* out_bf16,
    unsigned char* out_fp8, const int* row_order, long long nrows, float reg,
    void* stream) {
    if (!scale || !ext || !base) return hipErrorInvalidValue;
    return launch_als_solve_fused<true>(
        k, fp8, indptr, indices, ext, factors, out_f32, out_bf16, out_fp8,
        row_order, nrows, reg, scale, base, stream);
}

template <bool WT>
static int launch_gramian(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* values, const void* factors, float* A_out, float* b_out,
    const int* row_order, long long nrows, float reg, const float* scale,
    const float* base, void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4, 5, 6, 7, 8>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (fp8)
            k_gramian<KT, true, WT>
                <<<grid_block(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, values, (const unsigned char*)factors,
                    A_out, b_out, row_order, nrows, reg, scale, base);
        else
            k_gramian<KT, false, WT>
                <<<grid_block(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, values, (const unsigned short*)factors,
                    A_out, b_out, row_order, nrows, reg, scale, base);
        return hipGetLastError();
    });
}

extern "C" int fma_gramian(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* values, const void* factors, float* A_out, float* b_out,
    const int* row_order, long long nrows, float reg, void* stream) {
    return launch_gramian<false>(k, fp8, indptr, indices, values, factors,
                                 A_out, b_out, row_order, nrows, reg, nullptr,
                                 nullptr, stream);
}

extern "C" int fma_gramian_w(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* scale, const float* ext, const float* base,
    const void* factors, float* A_out, float* b_out, const int* row_order,
    long long nrows, float reg, void* stream) {
    if (!scale || !ext || !base) return hipErrorInvalidValue;
    return launch_gramian<true>(k, fp8, indptr, indices, ext, factors, A_out,
                                b_out, row_order, nrows, reg, scale, base,
                                stream);
}

extern "C" int fma_cholesky_solve_ph(
    int k, const float* A_in, const float* b_in, float* x_out,
    long long nrows, int phases, void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4, 5, 6, 7, 8>(k / 16, [&](auto kt) {
        k_cholesky_solve<decltype(kt)::value>
            <<<grid_block(nrows), kBlock, 0, (hipStream_t)stream>>>(
                A_in, b_in, x_out, nrows, phases);
        return hipGetLastError();
    });
}

extern "C" int fma_cholesky_solve(
    int k, const float* A_in, const float* b_in, float* x_out,
    long long nrows, void* stream) {
    return fma_cholesky_solve_ph(k, A_in, b_in, x_out, nrows, 3, stream);
}

extern "C" int fma_ldl_solve_wave(
    int k, const float* A_in, const float* b_in, float* x_out,
    unsigned short* x_bf16, unsigned char* x_fp8, long long nrows,
    void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4>(k / 16, [&](auto kt) {
        k_ldl_solve_wave<decltype(kt)::value>
            <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                A_in, b_in, x_out, x_bf16, x_fp8, nrows);
        return hipGetLastError();
    });
}

// the intermediate ladder levels (PANEL, SUBST) exist for
// k_als_solve_wavefused only
extern "C" int fma_ldl_solve_wave_reg(
    int k, const float* A_in, const float* b_in, float* x_out,
    unsigned short* x_bf16, unsigned char* x_fp8, long long nrows,
    int variant, void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        return dispatch_ic<WREG_BC_SHFL, WREG_BC_HOIST>(variant, [&](auto bc) {
            k_ldl_solve_wave_reg<KT, decltype(bc)::value>
                <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    A_in, b_in, x_out, x_bf16, x_fp8, nrows);
            return hipGetLastError();
        });
    });
}

extern "C" int fma_als_solve_wavefused_db(
    int k, const long long* indptr, const int* indices, const float* values,
    const void* factors, float* out_f32, unsigned short* out_bf16,
    unsigned char* out_fp8, const int* row_order, long long nrows,
    float reg, int variant, void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        return dispatch_ic<WREG_BC_SHFL, WREG_BC_HOIST>(variant, [&](auto bc) {
            k_als_solve_wavefused_db<KT, decltype(bc)::value>
                <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, values, factors, out_f32, out_bf16,
                    out_fp8, row_order, nrows, reg);
            return hipGetLastError();
        });
    });
}

extern "C" int fma_als_solve_wavefused(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* values, const void* factors, float* out_f32,
    unsigned short* out_bf16, unsigned char* out_fp8, const int* row_order,
    long long nrows, float reg, int variant, void* stream) {
    if (bad_shape(k, nrows)) return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        return dispatch_ic<WREG_BC_SHFL, WREG_BC_PANEL, WREG_BC_SUBST,
                           WREG_BC_HOIST>(variant, [&](auto bc) {
            constexpr int BC = decltype(bc)::value;
            if (fp8)
                k_als_solve_wavefused<KT, true, BC>
                    <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                        indptr, indices, values, factors, out_f32, out_bf16,
                        out_fp8, row_order, nrows, reg, nullptr, nullptr);
            else
                k_als_solve_wavefused<KT, false, BC>
                    <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                        indptr, indices, values, factors, out_f32, out_bf16,
                        out_fp8, row_order, nrows, reg, nullptr, nullptr);
            return hipGetLastError();
        });
    });
}

// weighted twin: the readlane broadcast level only (the other levels are
// measured ablations of the explicit kernel)
extern "C" int fma_als_solve_wavefused_w(
    int k, int fp8, const long long* indptr, const int* indices,
    const float* scale, const float* ext, const float* base,
    const void* factors, float* out_f32, unsigned short* out_bf16,
    unsigned char* out_fp8, const int* row_order, long long nrows, float reg,
    void* stream) {
    if (bad_shape(k, nrows) || !scale || !ext || !base)
        return hipErrorInvalidValue;
    return dispatch_ic<1, 2, 3, 4>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (fp8)
            k_als_solve_wavefused<KT, true, WREG_BC_HOIST, true>
                <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, ext, factors, out_f32, out_bf16,
                    out_fp8, row_order, nrows, reg, scale, base);
        else
            k_als_solve_wavefused<KT, false, WREG_BC_HOIST, true>
                <<<grid_wave(nrows), kBlock, 0, (hipStream_t)stream>>>(
                    indptr, indices, ext, factors, out_f32, out_bf16,
                    out_fp8, row_order, nrows, reg, scale, base);
        return hipGetLastError();
    });
}

// ---- factor Gram.  rows_per_part = 0: the launcher's choice; otherwise
// rounded up to a multiple of 32 (the stage chunk).
namespace {
inline long long factor_gram_rpp(long long n, int k, long long rows_per_part) {
    if (rows_per_part > 0) return (rows_per_part + 31) / 32 * 32;
    // enough parts to fill the machine, few enough that the workspace
    // (parts * k * k fp32) stays a small fraction of the table
    const long long max_parts = k <= 64 ? 1024 : 256;
    const long long rpp = (n + max_parts - 1) / max_parts;
    return rpp <= 32 ? 32 : (rpp + 31) / 32 * 32;
}
inline bool factor_gram_bad(long long n, int k, long long rows_per_part) {
    return n <= 0 || k <= 0 || k % 16 != 0 || k > 128 || rows_per_part < 0;
}
}  // namespace

extern "C" long long fma_factor_gram_rows_per_part(long long n, int k) {
    if (factor_gram_bad(n, k, 0)) return -1;
    return factor_gram_rpp(n, k, 0);
}

extern "C" long long fma_factor_gram_workspace_bytes(long long n, int k,
                                                     long long rows_per_part) {
    if (factor_gram_bad(n, k, rows_per_part)) return -1;
    const long long rpp = factor_gram_rpp(n, k, rows_per_part);
    return (n + rpp - 1) / rpp * (long long)k * k * 4;
}

namespace {
// rows == nullptr: the whole table, n rows; else the n-entry row list
int factor_gram_launch(int k, int fp8, const void* factors, const int* rows,
                       long long n, long long rows_per_part, float* G,
                       void* workspace, long long workspace_bytes,
                       void* stream) {
    const long long need = fma_factor_gram_workspace_bytes(n, k, rows_per_part);
    if (need < 0 || workspace_bytes < need || !workspace)
        return hipErrorInvalidValue;
    const long long rpp = factor_gram_rpp(n, k, rows_per_part);
    const long long parts = (n + rpp - 1) / rpp;
    return dispatch_ic<1, 2, 3, 4, 5, 6, 7, 8>(k / 16, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        auto launch = [&](auto f8, auto rw) {
            constexpr bool F8 = decltype(f8)::value;
            constexpr bool RW = decltype(rw)::value;
            k_factor_gram<KT, F8, RW>
                <<<grid_wave(parts), kBlock, 0, (hipStream_t)stream>>>(
                    (const typename GatherT<F8>::elem*)factors, rows,
                    (float*)workspace, n, rpp, parts);
        };
        using T = std::true_type;
        using F = std::false_type;
        if (rows) { if (fp8) launch(T{}, T{}); else launch(F{}, T{}); }
        else      { if (fp8) launch(T{}, F{}); else launch(F{}, F{}); }
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        k_factor_gram_reduce<KT>
            <<<dim3((k * k + 255) / 256), kBlock, 0, (hipStream_t)stream>>>(
                (const float*)workspace, G, parts);
        return hipGetLastError();
    });
}
}  // namespace

extern "C" int fma_factor_gram(int k, int fp8, const void* factors,
                               long long n, long long rows_per_part,
                               float* G, void* workspace,
                               long long workspace_bytes, void* stream) {
    return factor_gram_launch(k, fp8, factors, nullptr, n, rows_per_part, G,
                              workspace, workspace_bytes, stream);
}

extern "C" int fma_factor_gram_rows(int k, int fp8, const void* factors,
                                    long long ntable, const int* rows,
                                    long long nlist, long long rows_per_part,
                                    float* G, void* workspace,
                                    long long workspace_bytes, void* stream) {
    if (!rows || ntable <= 0 || ntable > 0x7fffffffLL)
        return hipErrorInvalidValue;
    return factor_gram_launch(k, fp8, factors, rows, nlist, rows_per_part, G,
                              workspace, workspace_bytes, stream);
}

extern "C" int fma_mfma_probe_f32(const float* A, const float* B, float* D,
                                  void* stream) {
    k_mfma_probe_f32<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(A, B, D);
    return hipGetLastError();
}

extern "C" int fma_mfma_probe_bf16(const unsigned short* Xt,
                                   const unsigned short* Yt, float* C,
                                   void* stream) {
    k_mfma_probe_bf16<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(Xt, Yt,
                                                                     C);
    return hipGetLastError();
}

extern "C" int fma_mfma_probe_fp8(const unsigned char* Xt,
                                  const unsigned char* Yt, float* C,
                                  void* stream) {
    k_mfma_probe_fp8<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(Xt, Yt,
                                                                    C);
    return hipGetLastError();
}
