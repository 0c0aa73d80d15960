// Shared device-side machinery for the ALS kernels (included by
// als_kernels.hip and debug_kernels.hip).  See als_kernels.hip for the
// design commentary.
#pragma once

#include <type_traits>

// ---------------------------------------------------------------- geometry

template <int KT> struct Geo {
    static constexpr int K = 16 * KT;
    static constexpr int NA = KT * (KT + 1) / 2;             // upper-triangle tiles
    static constexpr int TILES = NA + KT;                    // + EXT (b) tiles
    static constexpr int SLOTS = (TILES + 3) / 4;            // acc tiles per wave
    // transposed stage: Gt[K+16 rows][32 ratings], 96-B row stride (24
    // dwords: 16 used + 8 pad) -> the per-fragment ds_read_b128 is bank-
    // conflict-free across each 16-lane group
    static constexpr int TROW = 96;
    static constexpr int STAGE_BYTES = (K + 16) * TROW;
    // fp8 e4m3 stage: same Gt image at 1 byte/element, 40-B row stride
    // (10 dwords: 8 used + 2 pad).  Fragment reads are ds_read_b64; with
    // stride 10 dwords the 16 rows of a tile hit 16 distinct even banks
    // (gcd(10,32)=2) and the b64 pair fills the odd companions -> all 32
    // banks exactly once per 16-lane group.
    static constexpr int TROW8 = 40;
    static constexpr int STAGE8_BYTES = (K + 16) * TROW8;
    // multi-chunk staging (r2): wave w gathers chunk round*NCH+w into its
    // OWN stage buffer, so NCH chunks of 32 ratings are in flight per
    // round — the r1 kernel was chunk-turnaround latency bound (88.7%
    // wait-any with ~4 outstanding loads on one staging wave; halving the
    // gathered bytes with fp8 changed nothing).  NCH trades LDS (and thus
    // blocks/CU) for memory-level parallelism: bf16 buffers are 2.4x the
    // fp8 size, so bf16 stages 2 chunks per round and fp8 4.
    static constexpr int NCH_BF16 = 2;
    static constexpr int NCH_FP8 = 4;
    static constexpr int STAGE_TOTAL = NCH_BF16 * STAGE_BYTES;
    static constexpr int STAGE8_TOTAL = NCH_FP8 * STAGE8_BYTES;
    static constexpr int A_BYTES = K * (K + 1) * 4;
    static constexpr int CHOL_BYTES = A_BYTES + 8 * K + 16 * 16 * 4;
    static constexpr int SMEM = (NCH_BF16 * STAGE_BYTES > CHOL_BYTES)
                                    ? NCH_BF16 * STAGE_BYTES : CHOL_BYTES;
    static constexpr int SMEM8 = (NCH_FP8 * STAGE8_BYTES > CHOL_BYTES)
                                     ? NCH_FP8 * STAGE8_BYTES : CHOL_BYTES;
    // triangular A image (block solver): only the NA lower-triangle 16x16
    // tiles, row stride 17 (4-B-aligned rows; 17 coprime to 32 -> fully
    // conflict-free column walks; every solver access is scalar f32).  At
    // K=128 the image is 39.2 KB and the whole fused block (A + b hi/lo +
    // xbuf = 40.7 KB) fits FOUR blocks per CU's 160 KB LDS — r2 change:
    // LDT 18 + 1 KB colbuf scratch made it 43.5 KB = 3 blocks/CU.
    static constexpr int LDT = 17;
    static constexpr int TSZ = 16 * LDT;                     // floats per tile
    static constexpr int A_TRI_FLOATS = NA * TSZ;
    // + bhi/blo (2K floats) + xbuf (K floats)
    static constexpr int CHOL_TRI_BYTES = A_TRI_FLOATS * 4 + 12 * K;
    static constexpr int SMEM_TRI = (STAGE_TOTAL > CHOL_TRI_BYTES)
                                        ? STAGE_TOTAL : CHOL_TRI_BYTES;
    static constexpr int SMEM8_TRI = (STAGE8_TOTAL > CHOL_TRI_BYTES)
                                         ? STAGE8_TOTAL : CHOL_TRI_BYTES;
};

// fragment element type per gather precision
template <bool FP8> struct FragT { using type = bf16x8; };
template <> struct FragT<true> { using type = fp8x8; };

// storage element of a factor image per gather precision (the gathered
// factors and the low-precision copy of the solution): bf16 words or e4m3
// bytes
template <bool FP8> struct GatherT { using elem = unsigned short; };
template <> struct GatherT<true> { using elem = unsigned char; };

// triangular tile offset: tile (I,J), I >= J
DEV_INLINE constexpr int tri_off(int I, int J) {
    return (I * (I + 1)) / 2 + J;
}

// inverse: the tile-row I of linear lower-triangle index t
DEV_INLINE constexpr int lo_tile_i(int t) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    return i;
}

// ------------------------------------------------------------------ stage
// Gather one chunk's 32 factor rows (+ rating hi/lo EXT rows) into the
// TRANSPOSED Gt image — WAVE-LOCAL: the caller points each wave at its own
// stage buffer so NCH chunks gather concurrently (Geo::NCH_* rationale).
// bf16: task (q = rating quad, c8 = column oct) loads 4x16B row pieces and
// writes 8 ds_write_b64 transposed columns.  fp8: task (q, c16) loads
// 4x16B row pieces (a whole k<=64 e4m3 row is ONE 16-B load x4 lanes) and
// writes 16 ds_write_b32 transposed columns.  nrem = ratings left in the
// entity (rows >= nrem zero-filled).  The pieces: stage_gather4 (loads),
// stage_gather_w (+ transpose and LDS writes), stage_ext_load /
// stage_ext_commit (EXT rows, one rating per lane), stage_chunk_w (one
// whole chunk), stage_zero_pad (pad rows).
//
// WT (weighted normal equations, docs/KERNELS.md "Implicit feedback"): each
// gathered row is rescaled by its rating's scale[] entry between the gather
// and the transpose -- dequantise, ONE fp32 multiply, round back to the
// gather dtype (RNE) -- and ``values`` carries ext[] for the EXT rows.  The
// scale address depends on the rating's position only, so its load issues
// with the index loads: one 4-byte load per row piece, no second gather
// round.  IDENT (k_factor_gram): the chunk is rows base.. of the table
// itself (no index list, no EXT rows).  WIDEN (bf16 stage only): the table
// holds e4m3 bytes, widened exactly to bf16 as they are gathered.

typedef float stage_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 stage_bf16x2 __attribute__((ext_vector_type(2)));

// e4m3 saturation of f2fp8 (finite values clamp to +-448, NaN/inf pass)
DEV_INLINE float stage_fp8_sat(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u & 0x7f800000u) != 0x7f800000u
               ? __builtin_amdgcn_fmed3f(x, 448.0f, -448.0f) : x;
}

// four e4m3 bytes times s, re-rounded: per byte f2fp8(fp82f(b) * s)
DEV_INLINE unsigned stage_rescale_fp8x4(unsigned w, float s) {
    const stage_f32x2 s2 = {s, s};
    stage_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false) * s2;
    stage_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) * s2;
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(stage_fp8_sat(lo.x),
                                            stage_fp8_sat(lo.y), 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(stage_fp8_sat(hi.x),
                                        stage_fp8_sat(hi.y), r, true);
    return (unsigned)r;
}

// two bf16 words times s, re-rounded (RNE, v_cvt_pk_bf16_f32)
DEV_INLINE unsigned stage_rescale_bf16x2(unsigned d, float s) {
    const stage_f32x2 v = {__builtin_bit_cast(float, d << 16),
                           __builtin_bit_cast(float, d & 0xffff0000u)};
    const stage_f32x2 s2 = {s, s};
    return __builtin_bit_cast(
        unsigned, __builtin_convertvector(v * s2, stage_bf16x2));
}

// eight e4m3 bytes as eight bf16 words (exact), with the scalar helpers:
// k_factor_gram is a small memory-bound pass
DEV_INLINE uint4 stage_widen_fp8x8(uint2 raw) {
    unsigned out[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const unsigned w = (h < 2 ? raw.x : raw.y) >> (16 * (h & 1));
        out[h] = (unsigned)f2bf(fp82f((unsigned char)(w & 0xffu)))
                 | ((unsigned)f2bf(fp82f((unsigned char)((w >> 8) & 0xffu)))
                    << 16);
    }
    return uint4{out[0], out[1], out[2], out[3]};
}

template <bool FP8>
DEV_INLINE uint4 stage_rescale_piece(uint4 x, float s) {
    if constexpr (FP8)
        return uint4{stage_rescale_fp8x4(x.x, s), stage_rescale_fp8x4(x.y, s),
                     stage_rescale_fp8x4(x.z, s), stage_rescale_fp8x4(x.w, s)};
    else
        return uint4{stage_rescale_bf16x2(x.x, s),
                     stage_rescale_bf16x2(x.y, s),
                     stage_rescale_bf16x2(x.z, s),
                     stage_rescale_bf16x2(x.w, s)};
}

// An empty statement the optimizer can neither duplicate nor merge.
#define STAGE_NO_SINK() asm volatile("")

// One gather task's four row pieces: ratings row0..row0+3 counted from CSR
// position ``base``, 16 bytes (WIDEN: 8) at byte offset ``coff`` of each
// ROWB-byte factor row.  ``base`` and ``nrem`` (ratings left from base on)
// are WAVE-UNIFORM; row0 is the lane's own.
//
// full -- wave-uniform too, and it promises that every rating any lane of
// the wave asks for in this call is present: the task's four consecutive
// indices (WT: and scales) arrive as ONE 16-byte load each, then the four
// row loads issue back to back.  Two waits, no per-row branch, no zero
// fill.  The CSR offset is arbitrary, so the wide loads are only 4-byte
// aligned (memcpy spells that out).
//
// Otherwise every row is guarded as before: a row past the entity's range
// is neither indexed nor loaded -- the last entity's range ends with the
// allocation, so nothing wide may reach past it -- and stages as zeros.
template <int ROWB, bool WT, bool IDENT, bool WIDEN>
DEV_INLINE void stage_gather4(uint4 (&v)[4], float (&sc)[4],
                              const int* __restrict__ indices,
                              const char* __restrict__ factors,
                              const float* __restrict__ scale,
                              long long base, int nrem, int row0, int coff,
                              bool full) {
    if constexpr (!IDENT && !WIDEN) {
        if (full) {
            int idx[4];
            __builtin_memcpy(idx, indices + base + (unsigned)row0, 16);
            if constexpr (WT)
                __builtin_memcpy(sc, scale + base + (unsigned)row0, 16);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                v[m] = *(const uint4*)(factors + (long long)idx[m] * ROWB
                                       + coff);
            // Ends the block with something the guarded path has no twin
            // of: the optimizer otherwise sinks the last row's load out of
            // both paths into one guarded block, behind a wait of its own.
            STAGE_NO_SINK();
            return;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint4 x = {0, 0, 0, 0};
        const int row = row0 + m;
        if (row < nrem) {
            long long col;
            if constexpr (IDENT) col = base + row;
            else col = indices[base + (unsigned)row];
            if constexpr (WIDEN)
                x = stage_widen_fp8x8(
                    *(const uint2*)(factors + col * (long long)ROWB + coff));
            else
                x = *(const uint4*)(factors + col * (long long)ROWB + coff);
            if constexpr (WT) sc[m] = scale[base + (unsigned)row];
        }
        v[m] = x;
    }
}

// 4x4 byte transpose of one dword of four row pieces: out[c] holds byte c
// of a0..a3 (a0 in the low byte).  Two-stage v_perm_b32 butterfly, 8
// permutes for 4 words: stage one interleaves the bytes of (a0, a1) and of
// (a2, a3), stage two gathers the halfwords.  v_perm_b32 selects bytes 0-3
// from its SECOND source and 4-7 from its first.
DEV_INLINE void stage_transpose4x4_b8(unsigned a0, unsigned a1, unsigned a2,
                                      unsigned a3, unsigned* out) {
    const unsigned p01l = __builtin_amdgcn_perm(a1, a0, 0x05010400u);
    const unsigned p01h = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
    const unsigned p23l = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
    const unsigned p23h = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    out[0] = __builtin_amdgcn_perm(p23l, p01l, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(p23l, p01l, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(p23h, p01h, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(p23h, p01h, 0x07060302u);
}

// The gather + transpose of one chunk (no EXT rows) by NLANES lanes
// (``lane`` counts from 0 within them).  The chunk is ratings crow0 ..
// crow0+31 counted from CSR position ``base``; base, nrem and full as in
// stage_gather4, crow0 may differ between the lanes of a wave (split-wave
// staging: one half per chunk).
template <int KT, bool FP8, int NLANES = WAVE, bool WT = false,
          bool IDENT = false, bool WIDEN = false>
DEV_INLINE void stage_gather_w(char* buf,
                               const int* __restrict__ indices,
                               const void* __restrict__ factors_v,
                               long long base, int nrem, int lane, int crow0,
                               bool full,
                               const float* __restrict__ scale = nullptr) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    const char* factors = (const char*)factors_v;
    if constexpr (FP8) {
        constexpr int NT = 8 * (K / 16);
        for (int t = lane; t < NT; t += NLANES) {
            const int q = t & 7, c16 = t >> 3;
            uint4 v[4];
            [[maybe_unused]] float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            stage_gather4<K, WT, IDENT, false>(v, sc, indices, factors, scale,
                                               base, nrem, crow0 + 4 * q,
                                               c16 * 16, full);
            if constexpr (WT) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    v[m] = stage_rescale_piece<FP8>(v[m], sc[m]);
            }
            char* rb = buf + (long long)(16 * c16) * TROW + q * 4;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                unsigned wd[4];
                stage_transpose4x4_b8((&v[0].x)[d], (&v[1].x)[d],
                                      (&v[2].x)[d], (&v[3].x)[d], wd);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    *(unsigned*)(rb + (long long)(4 * d + c) * TROW) = wd[c];
            }
        }
    } else {
        constexpr int NT = 8 * (K / 8);
        for (int t = lane; t < NT; t += NLANES) {
            const int q = t & 7, c8 = t >> 3;
            uint4 v[4];
            [[maybe_unused]] float sc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            stage_gather4<(WIDEN ? K : 2 * K), WT, IDENT, WIDEN>(
                v, sc, indices, factors, scale, base, nrem, crow0 + 4 * q,
                WIDEN ? c8 * 8 : c8 * 16, full);
            if constexpr (WT) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    v[m] = stage_rescale_piece<FP8>(v[m], sc[m]);
            }
            char* rb = buf + (long long)(8 * c8) * TROW + q * 8;
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const unsigned d0 = (&v[0].x)[cc >> 1], d1 = (&v[1].x)[cc >> 1];
                const unsigned d2 = (&v[2].x)[cc >> 1], d3 = (&v[3].x)[cc >> 1];
                unsigned lo, hi;
                if (cc & 1) {
                    lo = (d0 >> 16) | (d1 & 0xffff0000u);
                    hi = (d2 >> 16) | (d3 & 0xffff0000u);
                } else {
                    lo = (d0 & 0xffffu) | (d1 << 16);
                    hi = (d2 & 0xffffu) | (d3 << 16);
                }
                *(uint2*)(rb + (long long)cc * TROW) = uint2{lo, hi};
            }
        }
    }
}

// The rating hi/lo EXT rows K, K+1, ONE RATING PER LANE: the lane that
// owns rating r of the chunk loads it, converts it once and places its hi
// and lo element (e4m3 byte / bf16 halfword) itself.  A wave-level
// instruction costs the same with 8 live lanes as with 32, so the
// conversion runs once per chunk instead of four times in series.
//
// The load comes first and the commit last in a staging call, so the value
// arrives behind the gather's own waits.  ``row`` is the rating's position
// counted from the wave-uniform ``base``; one past the entity's range
// (row >= nrem) is not loaded and stages as 0; full as in stage_gather4.
// WT passes ext[] as ``values``.
DEV_INLINE float stage_ext_load(const float* __restrict__ values,
                                long long base, int nrem, int row,
                                bool full) {
    float x = 0.0f;
    if (full) {
        x = values[base + (unsigned)row];
        STAGE_NO_SINK();
    } else if (row < nrem) {
        x = values[base + (unsigned)row];
    }
    return x;
}

template <int KT, bool FP8>
DEV_INLINE void stage_ext_commit(char* buf, int r, float x) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    if constexpr (FP8) {
        const unsigned char hb = f2fp8(x);
        const unsigned char lb = f2fp8(x - fp82f(hb));
        *(unsigned char*)(buf + (long long)K * TROW + r) = hb;
        *(unsigned char*)(buf + (long long)(K + 1) * TROW + r) = lb;
    } else {
        const unsigned short h = f2bf(x);
        const unsigned short l = f2bf(x - bf2f(h));
        *(unsigned short*)(buf + (long long)K * TROW + r * 2) = h;
        *(unsigned short*)(buf + (long long)(K + 1) * TROW + r * 2) = l;
    }
}

// The EXT rows the earlier way: 8 lanes convert four ratings each and write
// whole words.  Kept for the one instantiation (EXT8 below) that the
// per-lane form pushes over a register-allocation cliff.
template <int KT, bool FP8>
DEV_INLINE void stage_ext_quad_w(char* buf, const float* __restrict__ values,
                                 long long base, int nrem, int lane) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    if constexpr (FP8) {
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
        *(unsigned*)(buf + (long long)K * TROW + lane * 4) = h;
        *(unsigned*)(buf + (long long)(K + 1) * TROW + lane * 4) = l;
    } else {
        unsigned h2[2] = {0, 0}, l2[2] = {0, 0};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = 4 * lane + m;
            const float r = (row < nrem) ? values[base + row] : 0.0f;
            const unsigned short h = f2bf(r);
            const unsigned short l = f2bf(r - bf2f(h));
            h2[m >> 1] |= ((unsigned)h) << (16 * (m & 1));
            l2[m >> 1] |= ((unsigned)l) << (16 * (m & 1));
        }
        *(uint2*)(buf + (long long)K * TROW + lane * 8) = uint2{h2[0], h2[1]};
        *(uint2*)(buf + (long long)(K + 1) * TROW + lane * 8) =
            uint2{l2[0], l2[1]};
    }
}

// Gather + EXT rows of one chunk (ratings base.. of the CSR, nrem left) by
// NLANES >= 32 lanes (``lane`` counts from 0 within them); nrem must be
// uniform over those lanes' waves.  WIDE: take the unguarded path on a
// full chunk and load the rating ahead of the gather.  It holds four
// indices, four row pieces and the rating at once, which cost the block
// kernels and the single-chunk bf16 wave-fused kernel registers they do
// not have (a wave of occupancy at k = 112 / 128, a spill at k = 64), so
// those keep the guarded gather and stage the rating before it.
// EXT8: the 8-lane EXT conversion (stage_ext_quad_w).  With one rating per
// lane the bf16 k = 112 block-fused kernel allocates 131 VGPRs instead of
// 127 and drops from 4 waves per SIMD to 3; every other instantiation
// keeps its occupancy.
template <int KT, bool FP8, int NLANES = WAVE, bool WT = false,
          bool IDENT = false, bool WIDEN = false, bool WIDE = false,
          bool EXT8 = false>
DEV_INLINE void stage_chunk_w(char* buf,
                              const int* __restrict__ indices,
                              const float* __restrict__ values,
                              const void* __restrict__ factors_v,
                              long long base, int nrem, int lane,
                              const float* __restrict__ scale = nullptr) {
    static_assert(NLANES >= 32, "the EXT rows take 32 lanes");
    const bool full = WIDE && !IDENT && nrem >= 32;
    [[maybe_unused]] float xr = 0.0f;
    if constexpr (!IDENT && EXT8) {
        static_assert(!WIDE, "EXT8 goes with the guarded gather");
        if (lane < 8) stage_ext_quad_w<KT, FP8>(buf, values, base, nrem, lane);
    } else if constexpr (!IDENT) {
        if (lane < 32) {
            xr = stage_ext_load(values, base, nrem, lane, full);
            if constexpr (!WIDE) stage_ext_commit<KT, FP8>(buf, lane, xr);
        }
    }
    stage_gather_w<KT, FP8, NLANES, WT, IDENT, WIDEN>(
        buf, indices, factors_v, base, nrem, lane, 0, full, scale);
    if constexpr (!IDENT && WIDE) {
        if (lane < 32) stage_ext_commit<KT, FP8>(buf, lane, xr);
    }
}

// Zero the never-restaged EXT pad rows K+2..K+15 of one stage buffer with
// 16-byte stores: the 14 rows are one contiguous, 16-byte-aligned range
// ((K+2)*TROW and TROW*14 are multiples of 16 for both row strides; the
// rows' own pad bytes inside it are never read).  ``i`` / ``stride``: this
// thread's index and the thread count.
template <int KT, bool FP8>
DEV_INLINE void stage_zero_pad(char* buf, int i, int stride) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    constexpr int N16 = 14 * TROW / 16;
    static_assert((14 * TROW) % 16 == 0 && ((K + 2) * TROW) % 16 == 0,
                  "pad rows must be a 16-byte-aligned range");
    char* pad = buf + (long long)(K + 2) * TROW;
    for (; i < N16; i += stride)
        *(uint4*)(pad + (long long)i * 16) = uint4{0u, 0u, 0u, 0u};
}

// ... of all NCH stage buffers once per entity (block-wide).
template <int KT, bool FP8, int NCH>
DEV_INLINE void stage_zero_pad_all(char* smem) {
    constexpr int K = Geo<KT>::K;
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    constexpr int SB = (K + 16) * TROW;
#pragma unroll
    for (int b = 0; b < NCH; ++b)
        stage_zero_pad<KT, FP8>(smem + (long long)b * SB, threadIdx.x, 256);
}

// ------------------------------------------------------------- frag reads
// ONE ds_read per fragment (b128 bf16 / b64 fp8): lane l reads
// Gt[t*16 + (l&15)] [ratings 8g..8g+7] (g = l>>4) — the A/B operands share
// one (lane, element) map and the Gramian contracts over the rating axis,
// so any consistent hardware lane->k map yields the same A (validated by
// tests/test_gpu_mfma.py probes for both dtypes).
template <int KT, bool FP8>
DEV_INLINE void read_frags(const char* buf, int lane,
                           typename FragT<FP8>::type* frag) {
    constexpr int TROW = FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW;
    constexpr int FB = FP8 ? 8 : 16;
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int t = 0; t <= KT; ++t)
        frag[t] = *(const typename FragT<FP8>::type*)(
            buf + (long long)(t * 16 + li) * TROW + g * FB);
}

// --------------------------------------------------------------- MFMA loop

template <int KT, int W, bool FP8, int S = 0>
DEV_INLINE void mfma_tiles(const typename FragT<FP8>::type* frag, f32x4* acc) {
    if constexpr (S < Geo<KT>::SLOTS) {
        constexpr int t = W + 4 * S;
        if constexpr (t < Geo<KT>::TILES) {
            constexpr int NA = Geo<KT>::NA;
            constexpr int p = (t < NA) ? up_tile_p(t, KT) : (t - NA);
            constexpr int q = (t < NA) ? up_tile_q((t < NA) ? t : 0, KT) : KT;
            if constexpr (FP8) {
                acc[S] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                    frag[p], frag[q], acc[S], 0, 0, 0);
            } else {
                acc[S] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    frag[p], frag[q], acc[S], 0, 0, 0);
            }
        }
        mfma_tiles<KT, W, FP8, S + 1>(frag, acc);
    }
}

// Spill accumulators to the LDS A/b images (C/D map: row=(l>>4)*4+r, col=l&15).
template <int KT, int W, int S = 0>
DEV_INLINE void write_acc(const f32x4* acc, float* A, float* bhi, float* blo,
                          int lane) {
    if constexpr (S < Geo<KT>::SLOTS) {
        constexpr int t = W + 4 * S;
        if constexpr (t < Geo<KT>::TILES) {
            constexpr int K = Geo<KT>::K;
            constexpr int NA = Geo<KT>::NA;
            constexpr int p = (t < NA) ? up_tile_p(t, KT) : (t - NA);
            constexpr int q = (t < NA) ? up_tile_q((t < NA) ? t : 0, KT) : KT;
            const int g = lane >> 4, li = lane & 15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = p * 16 + g * 4 + r;
                if constexpr (q == KT) {       // EXT: b tile, cols 0/1 = hi/lo
                    if (li == 0) bhi[row] = acc[S][r];
                    else if (li == 1) blo[row] = acc[S][r];
                } else {
                    const int col = q * 16 + li;
                    A[row * (K + 1) + col] = acc[S][r];
                    if constexpr (p != q) A[col * (K + 1) + row] = acc[S][r];
                }
            }
        }
        write_acc<KT, W, S + 1>(acc, A, bhi, blo, lane);
    }
}

// write_acc into the TRIANGULAR tile image: the accumulated upper tile
// (p,q), p <= q, lands TRANSPOSED in lower tile (q,p); diagonal tiles land
// in full (their upper half doubles as the panel-factorization scratch).
template <int KT, int W, int S = 0>
DEV_INLINE void write_acc_tri(const f32x4* acc, float* A, float* bhi,
                              float* blo, int lane) {
    if constexpr (S < Geo<KT>::SLOTS) {
        constexpr int t = W + 4 * S;
        if constexpr (t < Geo<KT>::TILES) {
            constexpr int NA = Geo<KT>::NA;
            constexpr int LDT = Geo<KT>::LDT;
            constexpr int TSZ = Geo<KT>::TSZ;
            constexpr int p = (t < NA) ? up_tile_p(t, KT) : (t - NA);
            constexpr int q = (t < NA) ? up_tile_q((t < NA) ? t : 0, KT) : KT;
            const int g = lane >> 4, li = lane & 15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lrow = g * 4 + r;
                if constexpr (q == KT) {       // EXT: b tile, cols 0/1 = hi/lo
                    if (li == 0) bhi[p * 16 + lrow] = acc[S][r];
                    else if (li == 1) blo[p * 16 + lrow] = acc[S][r];
                } else if constexpr (p == q) {
                    A[tri_off(p, p) * TSZ + lrow * LDT + li] = acc[S][r];
                } else {                        // store transposed in (q,p)
                    A[tri_off(q, p) * TSZ + li * LDT + lrow] = acc[S][r];
                }
            }
        }
        write_acc_tri<KT, W, S + 1>(acc, A, bhi, blo, lane);
    }
}

// ------------------------------------------------------ in-LDS LDL^T/solve

// In-place LDL^T elimination of the triangular LDS image (lower 16x16
// tiles at tri_off, row stride Geo::LDT), 16-column panels, 256-thread
// block version (k up to 128; the k<=64 wave solvers in als_kernels.hip are
// the same algorithm without barriers):
//   (a) panel factorization: wave 0 factors the whole panel slab in
//       registers -- lane owns rows lane and lane+64, pivot column values
//       broadcast by __shfl, no barriers inside the panel.  Rows above the
//       panel have no storage in the triangular image and sit it out;
//   (b) trailing update as f32 MFMA 16x16 tiles (v_mfma_f32_16x16x4_f32,
//       exact fp32), tiles round-robined over the 4 waves, all 64 lanes
//       live.  Diagonal tiles are kept in full: their upper halves are
//       never-read scratch.
template <int K>
DEV_INLINE void cholesky_lds_tri(float* A) {
    constexpr int NP = K / 16;
    constexpr int LDT = Geo<K / 16>::LDT;
    constexpr int TSZ = Geo<K / 16>::TSZ;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g4 = lane >> 4;
#pragma unroll 1
    for (int pi = 0; pi < NP; ++pi) {
        const int P0 = 16 * pi;
        if (w == 0) {
            float sa[16], sb[16];
            const bool av = lane < K && lane >= P0;
            const bool bv = (K > 64) && (lane + 64 < K) && (lane + 64 >= P0);
            float* rsa = A + tri_off(lane >> 4, pi) * TSZ + (lane & 15) * LDT;
            float* rsb = A + tri_off((lane + 64) >> 4, pi) * TSZ
                         + (lane & 15) * LDT;
            if (av) {
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) sa[cc] = rsa[cc];
            }
            if (bv) {
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) sb[cc] = rsb[cc];
            }
#pragma unroll
            for (int jj = 0; jj < 15; ++jj) {
                const int j = P0 + jj;
                const bool jhi = j >= 64;
                const float dj = __shfl(jhi ? sb[jj] : sa[jj], j & 63, WAVE);
                const float dinv = dj > 0.0f ? 1.0f / dj : 0.0f;
                const float la = sa[jj] * dinv, lb = sb[jj] * dinv;
#pragma unroll
                for (int cc = jj + 1; cc < 16; ++cc) {
                    const bool chi = P0 + cc >= 64;
                    const float colj = __shfl(chi ? sb[jj] : sa[jj],
                                              (P0 + cc) & 63, WAVE);
                    sa[cc] -= la * colj;
                    sb[cc] -= lb * colj;
                }
            }
            if (av) {
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) rsa[cc] = sa[cc];
            }
            if (bv) {
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) rsb[cc] = sb[cc];
            }
        }
        __syncthreads();
        if (pi == NP - 1) break;
        const float* Tpp = A + tri_off(pi, pi) * TSZ;
        float ndk[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = 4 * kk + g4;
            const float d = Tpp[c * LDT + c];
            ndk[kk] = d > 0.0f ? -1.0f / d : 0.0f;
        }
        int idx = 0;
#pragma unroll 1
        for (int rb = pi + 1; rb < NP; ++rb) {
            const float* TA = A + tri_off(rb, pi) * TSZ;
#pragma unroll 1
            for (int cb = pi + 1; cb <= rb; ++cb) {
                if ((idx++ & 3) != w) continue;
                const float* TB = A + tri_off(cb, pi) * TSZ;
                float* TC = A + tri_off(rb, cb) * TSZ;
                f32x4 acc;
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
        __syncthreads();
    }
}

// Blocked triangular solves over the LDL^T image, 256 threads: thread r
// owns row r's running value in a register; per 16-row block, the lanes of
// wave 0 run the sequential in-block substitution (shfl chain) and publish
// z through ``xbuf`` (LDS, >= K floats), then every thread applies the
// block's contribution to its row with 16 fma.  Writes x, and its bf16 /
// e4m3 image where ``xb_row`` / ``x8_row`` is non-null, straight to global.
template <int K>
DEV_INLINE void solve_lds_block_tri(const float* A, const float* b,
                                    float* xbuf, float* x_row,
                                    unsigned short* xb_row,
                                    unsigned char* x8_row = nullptr) {
    constexpr int NP = K / 16;
    constexpr int LDT = Geo<K / 16>::LDT;
    constexpr int TSZ = Geo<K / 16>::TSZ;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool own = tid < K;
    const int Ir = tid >> 4, lr = tid & 15;
    float acc = own ? b[tid] : 0.0f;
    const float dr = own ? A[tri_off(Ir, Ir) * TSZ + lr * LDT + lr] : 1.0f;
    const float invd = dr > 0.0f ? 1.0f / dr : 0.0f;
    // forward: (I + Ls) y = b, Ls[r][j] = A[r][j] / D_j
#pragma unroll 1
    for (int bi = 0; bi < NP; ++bi) {
        const int B0 = 16 * bi;
        const float* Tbb = A + tri_off(bi, bi) * TSZ;
        if (own && tid >= B0 && tid < B0 + 16) xbuf[tid] = acc;
        __syncthreads();
        if (w == 0) {  // in-block substitution on lanes 0..15
            const int r = B0 + (lane & 15);
            float v = (lane < 16 && r < K) ? xbuf[r] : 0.0f;
            float di = (lane < 16 && r < K)
                           ? Tbb[(lane & 15) * LDT + (lane & 15)] : 1.0f;
            di = di > 0.0f ? 1.0f / di : 0.0f;
#pragma unroll
            for (int t = 0; t < 15; ++t) {
                const float zt = __shfl(v, t, WAVE) * __shfl(di, t, WAVE);
                if (lane < 16 && lane > t && r < K)
                    v -= Tbb[(lane & 15) * LDT + t] * zt;
            }
            if (lane < 16 && r < K) xbuf[r] = v * di;  // z_j = y_j / D_j
        }
        __syncthreads();
        if (own && tid >= B0 + 16) {
            const float* Trb = A + tri_off(Ir, bi) * TSZ + lr * LDT;
            float s = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                s += Trb[cc] * xbuf[B0 + cc];
            acc -= s;
        } else if (own && tid >= B0 && tid < B0 + 16) {
            acc = xbuf[tid] * dr;  // recover y_j from z_j
        }
        __syncthreads();
    }
    // w = y / D
    acc *= invd;
    // backward: (I + Ls^T) x = w ; Ls^T[j][c] = A[c][j] / D_j
#pragma unroll 1
    for (int bi = NP - 1; bi >= 0; --bi) {
        const int B0 = 16 * bi;
        const float* Tbb = A + tri_off(bi, bi) * TSZ;
        if (own && tid >= B0 && tid < B0 + 16) xbuf[tid] = acc;
        __syncthreads();
        if (w == 0) {
            const int r = B0 + (lane & 15);
            float v = (lane < 16 && r < K) ? xbuf[r] : 0.0f;
            float di = (lane < 16 && r < K)
                           ? Tbb[(lane & 15) * LDT + (lane & 15)] : 1.0f;
            di = di > 0.0f ? 1.0f / di : 0.0f;
#pragma unroll
            for (int t = 15; t >= 1; --t) {
                const float xt = __shfl(v, t, WAVE);
                if (lane < 16 && lane < t && r < K)
                    v -= Tbb[t * LDT + (lane & 15)] * di * xt;
            }
            if (lane < 16 && r < K) xbuf[r] = v;
        }
        __syncthreads();
        if (own && tid < B0) {
            const float* Tbr = A + tri_off(bi, Ir) * TSZ + lr;
            float s = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc)
                s += Tbr[cc * LDT] * xbuf[B0 + cc];
            acc -= s * invd;
        } else if (own && tid >= B0 && tid < B0 + 16) {
            acc = xbuf[tid];
        }
        __syncthreads();
    }
    if (own) {
        x_row[tid] = acc;
        if (xb_row) xb_row[tid] = f2bf(acc);
        if (x8_row) x8_row[tid] = f2fp8(acc);
    }
}

// ------------------------------------------------- Gramian accumulation core
// Runs the multi-chunk stage->frag->MFMA loop and leaves A (mirrored, with
// lambda*n*I) + combined b in LDS.  Per round, wave w gathers chunk
// r0 + w into its own stage buffer (NCH chunks of gathers in flight), then
// all waves MFMA every staged chunk.  Returns n (ratings of this entity).
// WT: weighted normal equations -- ``values`` is ext[], rows are rescaled
// by ``scale`` in staging, and COMBINE adds the symmetric base matrix G0
// ([K][K] fp32, lower triangle read) to the finished image.
template <int KT, bool COMBINE = true, bool TRI = false, bool FP8 = false,
          bool WT = false>
DEV_INLINE int gramian_to_lds(char* smem,
                              const long long* __restrict__ indptr,
                              const int* __restrict__ indices,
                              const float* __restrict__ values,
                              const void* __restrict__ factors,
                              long long row, float reg,
                              const float* __restrict__ scale = nullptr,
                              const float* __restrict__ G0 = nullptr) {
    constexpr int K = Geo<KT>::K;
    constexpr int NCH = FP8 ? Geo<KT>::NCH_FP8 : Geo<KT>::NCH_BF16;
    constexpr int SB = (K + 16) * (FP8 ? Geo<KT>::TROW8 : Geo<KT>::TROW);
    const int tid = threadIdx.x, lane = tid & 63;
    // readfirstlane: make the wave id PROVABLY wave-uniform so the
    // per-wave tile switch compiles to scalar branches, not exec-mask
    // waterfalls around the MFMAs (cdna_hip_programming.md §5.5 T20;
    // the masked-MFMA form miscompiled the accumulator spills here).
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p0 = indptr[row];
    const int n = (int)(indptr[row + 1] - p0);
    if (n == 0) return 0;

    f32x4 acc[Geo<KT>::SLOTS];
#pragma unroll
    for (int s = 0; s < Geo<KT>::SLOTS; ++s) acc[s] = f32x4{0, 0, 0, 0};

    // team staging: a chunk's gather tasks need NT lanes at a 4-load
    // burst (r1: doubling the per-lane burst cost 13%); when NT > 64
    // (bf16 K=128) a TEAM of 2 waves stages one chunk together
    constexpr int NT = FP8 ? 8 * (K / 16) : K;
    constexpr int TW = (NT > WAVE) ? 2 : 1;       // waves per chunk team
    constexpr int NCHU = (NCH < 4 / TW) ? NCH : 4 / TW;
    stage_zero_pad_all<KT, FP8, NCHU>(smem);
    const int team = w / TW;
    const int tlane = (w % TW) * WAVE + lane;
    const int nchunks = (n + 31) >> 5;
    for (int r0 = 0; r0 < nchunks; r0 += NCHU) {
        if (team < NCHU && r0 + team < nchunks)
            stage_chunk_w<KT, FP8, TW * WAVE, WT, false, false, false,
                          /*EXT8=*/(!FP8 && KT == 7)>(
                smem + team * SB, indices, values, factors,
                p0 + (long long)(r0 + team) * 32, n - (r0 + team) * 32,
                tlane, scale);
        __syncthreads();
        const int ns = min(NCHU, nchunks - r0);
        for (int sc = 0; sc < ns; ++sc) {
            typename FragT<FP8>::type frag[KT + 1];
            read_frags<KT, FP8>(smem + sc * SB, lane, frag);
            switch (w) {
                case 0: mfma_tiles<KT, 0, FP8>(frag, acc); break;
                case 1: mfma_tiles<KT, 1, FP8>(frag, acc); break;
                case 2: mfma_tiles<KT, 2, FP8>(frag, acc); break;
                default: mfma_tiles<KT, 3, FP8>(frag, acc); break;
            }
        }
        __syncthreads();
    }

    float* A = (float*)smem;
    float* bhi = A + (TRI ? Geo<KT>::A_TRI_FLOATS : K * (K + 1));
    float* blo = bhi + K;
    if constexpr (TRI) {
        switch (w) {
            case 0: write_acc_tri<KT, 0>(acc, A, bhi, blo, lane); break;
            case 1: write_acc_tri<KT, 1>(acc, A, bhi, blo, lane); break;
            case 2: write_acc_tri<KT, 2>(acc, A, bhi, blo, lane); break;
            default: write_acc_tri<KT, 3>(acc, A, bhi, blo, lane); break;
        }
    } else {
        switch (w) {
            case 0: write_acc<KT, 0>(acc, A, bhi, blo, lane); break;
            case 1: write_acc<KT, 1>(acc, A, bhi, blo, lane); break;
            case 2: write_acc<KT, 2>(acc, A, bhi, blo, lane); break;
            default: write_acc<KT, 3>(acc, A, bhi, blo, lane); break;
        }
    }
    __syncthreads();
    if constexpr (WT && COMBINE) {
        // A += G0.  Element (r, c) reads G0[max][min]: the lower triangle
        // only, and the diagonal tiles' upper halves stay symmetric.
        if constexpr (TRI) {
            const int lr = tid >> 4, lc = tid & 15;   // one tile per pass
            int I = 0, J = 0;
            for (int t = 0; t < Geo<KT>::NA; ++t) {
                const int r = I * 16 + lr, c = J * 16 + lc;
                A[t * Geo<KT>::TSZ + lr * Geo<KT>::LDT + lc] +=
                    G0[max(r, c) * K + min(r, c)];
                if (++J > I) { ++I; J = 0; }
            }
        } else {
            for (int i = tid; i < K * K; i += 256) {
                const int r = i / K, c = i % K;
                A[r * (K + 1) + c] += G0[max(r, c) * K + min(r, c)];
            }
        }
        __syncthreads();
    }
    if (COMBINE && tid < K) {
        bhi[tid] += blo[tid];                       // combined b
        float* dp = TRI
            ? A + tri_off(tid >> 4, tid >> 4) * Geo<KT>::TSZ
                  + (tid & 15) * Geo<KT>::LDT + (tid & 15)
            : A + tid * (K + 1) + tid;
        float dd = *dp + reg * (float)n;
        if (dd <= 0.0f) dd = 1.0f;                  // degenerate guard
        *dp = dd;
    }
    __syncthreads();
    return n;
}

template <int KT, typename LP>
DEV_INLINE void write_zero_row(float* out_f32, LP* out_lowp, long long row) {
    constexpr int K = Geo<KT>::K;
    for (int c = threadIdx.x; c < K; c += 256) {
        out_f32[row * K + c] = 0.0f;
        if (out_lowp) out_lowp[row * K + c] = 0;
    }
}

// ------------------------------------------------------- launcher dispatch
// Host side: maps a runtime value onto the compile-time list VS.  ``f`` is a
// generic lambda called with std::integral_constant<int, V> for the V that
// equals ``v`` and returns the launch status; a value outside the list is
// hipErrorInvalidValue.  Nest two calls to pick (k/16, variant) pairs --
// only the listed combinations are instantiated.
template <int... VS, typename F>
inline hipError_t dispatch_ic(int v, F&& f) {
    hipError_t err = hipErrorInvalidValue;
    (void)((v == VS &&
            ((err = f(std::integral_constant<int, VS>{})), true)) || ...);
    return err;
}
