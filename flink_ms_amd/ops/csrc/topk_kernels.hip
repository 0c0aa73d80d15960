// Top-N recommendation kernels for MI355X (gfx950): fused Q.V^T scoring and
// per-query top-k selection.  No reference analog (ALSPredict.java only
// does point dots); the [queries][items] score matrix never exists in HBM.
// The rank-count kernels (K9, second half of this file) score with the same
// fragments and MFMA steps and count instead of select.
//
//   k_topk_partial  one WAVE owns (16-query tile) x (one chunk of the
//                   candidate list).  Q fragments stay in registers; per
//                   16-item tile each lane loads its B fragment straight from
//                   V[cand[base + (lane & 15)]] and ceil(k/32)
//                   v_mfma_f32_16x16x32_bf16 give 4 scores per lane
//                   (query = 4 (lane >> 4) + j, item = lane & 15).  Scores
//                   that beat the query's threshold and are not excluded are
//                   appended to a wave-private LDS list (capacity 2 KB
//                   entries per query); a full list is sorted down to topk
//                   and the threshold raised.  The chunk's sorted topk goes
//                   to workspace[q][chunk][.].
//   k_topk_merge    one wave per query runs its nchunks sorted partial lists
//                   through the same filter / list / sort, 64 lists at a
//                   time, leaving a list at its first key below threshold.
//
// Everything is selected on ONE 64-bit key per (score, row):
//   high word: the fp32 score mapped to an unsigned that orders like the
//              float (NaN -> 0, below -inf); low word: ~row.
// A larger key is a better candidate, so "score descending, lower row
// first" is plain unsigned order, keys of distinct rows are distinct, and
// the top-k set (hence the result) cannot depend on chunking or the grid.
// Key 0 is the padding entry (row -1, score -inf): ~row >= 2^31 for every
// real row, which is why the launcher bounds nv below 2^31.
//
// Waves never wait for each other: no block barriers, no global atomics.
// The lanes of a wave exchange list entries through LDS, ordered by
// TOPK_FENCE (the DS unit serves one wave's operations in issue order).

#include "common.hip.h"
#include "fma_api.h"

typedef unsigned long long u64;

#define TOPK_FENCE() __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

constexpr int TOPK_MERGE_CAP = 256;   // merge list: >= 128 kept + 64 new

DEV_INLINE u64 topk_key(float s, unsigned inv_row) {
    union { float f; unsigned u; } v;
    v.f = s + 0.0f;                        // -0 ties with +0
    unsigned hi;
    if ((v.u & 0x7fffffffu) > 0x7f800000u) hi = 0u;          // NaN: last
    else hi = (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
    return ((u64)hi << 32) | inv_row;
}

DEV_INLINE void topk_decode(u64 key, float* score, long long* row) {
    union { float f; unsigned u; } v;
    const unsigned hi = (unsigned)(key >> 32);
    if (key == 0ull) {
        v.u = 0xff800000u;                 // -inf
        *row = -1;
    } else {
        *row = (long long)(~(unsigned)key);
        if (hi == 0u) v.u = 0x7fc00000u;   // NaN
        else v.u = (hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi;
    }
    *score = v.f;
}

// Bitonic sort, descending, of the N keys at L by the GW lanes that share
// the list (gl = this lane's index among them).  Lists of different lane
// groups are disjoint, so the groups of a wave sort side by side.
template <int N, int GW>
DEV_INLINE void group_sort_desc(u64* L, int gl) {
    static_assert((N / 2) % GW == 0, "whole rounds of compare-exchanges");
    constexpr int IT = N / 2 / GW;
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            // all of a stage's loads before its stores: the pairs of one
            // stage are disjoint, and the LDS latency is paid once
            u64 a[IT], b[IT];
#pragma unroll
            for (int u = 0; u < IT; ++u) {
                const int t = gl + u * GW;
                const int i = 2 * t - (t & (stride - 1));
                a[u] = L[i];
                b[u] = L[i + stride];
            }
#pragma unroll
            for (int u = 0; u < IT; ++u) {
                const int t = gl + u * GW;
                const int i = 2 * t - (t & (stride - 1));
                const bool desc = (i & size) == 0;
                if ((a[u] < b[u]) == desc) {
                    L[i] = b[u];
                    L[i + stride] = a[u];
                }
            }
            TOPK_FENCE();
        }
    }
}

// One lane's 8 bf16 of a 32-wide k step: columns c0..c0+7 of ``row`` (null
// = an invalid tile slot), zero past k.  ``vec`` (k % 8 == 0 and 16-byte
// aligned bases) takes one 16-byte load.
DEV_INLINE bf16x8 topk_load_frag(const unsigned short* row, int k, int c0,
                                 bool vec) {
    bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row != nullptr && c0 < k) {
        if (vec) {
            f = *(const bf16x8*)(row + c0);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j < k) f[j] = (short)row[c0 + j];
        }
    }
    return f;
}

// Is ``row`` in the sorted slice excl_rows[lo, hi)?
DEV_INLINE bool topk_excluded(const long long* excl_rows, long long lo,
                              long long hi, long long row) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        const long long v = excl_rows[mid];
        if (v == row) return true;
        if (v < row) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// Sort the lists of queries 4g+j down to topk entries and raise their
// thresholds.  Wave-uniform control flow; ``force`` sorts every list (the
// chunk's end), otherwise only the j whose list outgrew topk somewhere.
template <int KB>
DEV_INLINE void topk_compact4(u64* L, int (&cnt)[4], u64 (&thr)[4], int topk,
                              int g, int li, bool force) {
    constexpr int CAP = 2 * KB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!force && !__any(cnt[j] > topk)) continue;
        u64* Lq = L + (4 * g + j) * CAP;
        for (int t = cnt[j] + li; t < CAP; t += 16) Lq[t] = 0ull;
        TOPK_FENCE();
        group_sort_desc<CAP, 16>(Lq, li);
        cnt[j] = cnt[j] < topk ? cnt[j] : topk;
        thr[j] = cnt[j] == topk ? Lq[topk - 1] : 0ull;
    }
}

template <int KB, int WPB>
__launch_bounds__(WPB * 64)
__global__ void k_topk_partial(const unsigned short* __restrict__ Q,
                               const unsigned short* __restrict__ V,
                               const long long* __restrict__ cand,
                               const long long* __restrict__ excl_ptr,
                               const long long* __restrict__ excl_rows,
                               u64* __restrict__ ws, long long nq,
                               long long nc, int k, int topk,
                               long long chunk, long long nchunks,
                               long long nqt, int vec) {
    constexpr int CAP = 2 * KB;
    __shared__ __align__(16) u64 lds[WPB * 16 * CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    const long long unit = (long long)blockIdx.x * WPB + wv;
    if (unit >= nqt * nchunks) return;     // waves are independent
    const long long qt = unit % nqt, ch = unit / nqt;
    const long long q0 = qt * 16;
    const long long cstart = ch * chunk;
    const long long cend = cstart + chunk < nc ? cstart + chunk : nc;
    u64* L = lds + wv * 16 * CAP;
    const int KS = (k + 31) >> 5;

    // A fragments: Q[q0 + li][32 s + 8 g + 0..7], resident for the chunk
    bf16x8 qf[4];
    {
        const unsigned short* qrow =
            q0 + li < nq ? Q + (q0 + li) * (long long)k : nullptr;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[s] = topk_load_frag(s < KS ? qrow : nullptr, k, 32 * s + 8 * g,
                                   vec);
    }

    int cnt[4] = {0, 0, 0, 0};
    u64 thr[4] = {0ull, 0ull, 0ull, 0ull};

    auto load_tile = [&](long long base, long long& r, bf16x8 (&vf)[4]) {
        const long long idx = base + li;
        r = -1;
        if (idx < cend) r = cand != nullptr ? cand[idx] : idx;
        const unsigned short* vrow = r >= 0 ? V + r * (long long)k : nullptr;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            vf[s] = topk_load_frag(s < KS ? vrow : nullptr, k,
                                   32 * s + 8 * g, vec);
    };

    long long r_cur;
    bf16x8 vf[4];
    load_tile(cstart, r_cur, vf);
    for (long long base = cstart; base < cend; base += 16) {
        // the next tile's loads fly while this one is scored and filtered
        long long r_nxt = -1;
        bf16x8 vn[4];
        load_tile(base + 16, r_nxt, vn);

        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < KS)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], vf[s],
                                                              acc, 0, 0, 0);
        const unsigned inv_row = ~(unsigned)r_cur;
        bool over = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long q = q0 + 4 * g + j;
            const u64 key = topk_key(acc[j], inv_row);
            bool pass = r_cur >= 0 && q < nq && key > thr[j];
            if (pass && excl_ptr != nullptr)
                pass = !topk_excluded(excl_rows, excl_ptr[q], excl_ptr[q + 1],
                                      r_cur);
            const u64 mask = __ballot(pass);
            if (mask != 0ull) {
                const unsigned bits = (unsigned)(mask >> (16 * g)) & 0xffffu;
                const int pos = cnt[j] + __popc(bits & ((1u << li) - 1u));
                if (pass) L[(4 * g + j) * CAP + pos] = key;
                cnt[j] += __popc(bits);
            }
            over = over || cnt[j] > CAP - 16;
        }
        // room for one more tile (16 entries) in every list, or compact
        if (__any(over)) {
            TOPK_FENCE();
            topk_compact4<KB>(L, cnt, thr, topk, g, li, false);
        }
        r_cur = r_nxt;
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = vn[s];
    }
    TOPK_FENCE();
    topk_compact4<KB>(L, cnt, thr, topk, g, li, true);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long q = q0 + 4 * g + j;
        if (q >= nq) continue;
        const u64* Lq = L + (4 * g + j) * CAP;
        u64* dst = ws + (q * nchunks + ch) * (long long)topk;
        for (int t = li; t < topk; t += 16)
            dst[t] = t < cnt[j] ? Lq[t] : 0ull;
    }
}

// One wave per query.  Lane l walks partial list c0 + l front to back, so a
// step looks at position t of 64 lists at once.  The lists are sorted and
// the threshold only rises: once no lane passes at some t, nothing further
// down these 64 lists can, and the wave moves on to the next 64 lists.
__launch_bounds__(256)
__global__ void k_topk_merge(const u64* __restrict__ ws,
                             float* __restrict__ out_scores,
                             long long* __restrict__ out_rows, long long nq,
                             long long nchunks, int topk) {
    constexpr int CAP = TOPK_MERGE_CAP;
    __shared__ __align__(16) u64 lds[4 * CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 4 + wv;
    if (q >= nq) return;
    u64* L = lds + wv * CAP;
    const u64* src = ws + q * nchunks * topk;
    int cnt = 0;
    u64 thr = 0ull;
    auto compact = [&]() {
        for (int t = cnt + lane; t < CAP; t += 64) L[t] = 0ull;
        TOPK_FENCE();
        group_sort_desc<CAP, 64>(L, lane);
        cnt = cnt < topk ? cnt : topk;
        thr = cnt == topk ? L[topk - 1] : 0ull;
    };
    for (long long c0 = 0; c0 < nchunks; c0 += 64) {
        const bool have = c0 + lane < nchunks;
        const u64* lp = src + (have ? c0 + lane : 0) * topk;
        u64 next = have ? lp[0] : 0ull;
        for (int t = 0; t < topk; ++t) {
            const u64 key = next;
            next = have && t + 1 < topk ? lp[t + 1] : 0ull;
            const bool pass = key > thr;   // padding (0) never passes
            const u64 mask = __ballot(pass);
            if (mask == 0ull) break;       // wave-uniform
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (pass) L[pos] = key;
            cnt += __popcll(mask);
            if (cnt > CAP - 64) {          // room for 64 more, or compact
                TOPK_FENCE();
                compact();
            }
        }
    }
    TOPK_FENCE();
    compact();
    for (int t = lane; t < topk; t += 64) {
        float s;
        long long r;
        topk_decode(t < cnt ? L[t] : 0ull, &s, &r);
        out_scores[q * topk + t] = s;
        out_rows[q * topk + t] = r;
    }
}

// ------------------------------------------------------------- launchers

static int topk_kb(int topk) {
    return topk <= 16 ? 16 : topk <= 32 ? 32 : topk <= 64 ? 64 : 128;
}

static bool topk_shape_ok(long long nq, long long nc, int topk,
                          long long chunk_items) {
    return nq >= 1 && nc >= 1 && nc < (1ll << 31) && topk >= 1 &&
           topk <= 128 && chunk_items >= 0;
}

// Chunk length the launcher picks: about 2048 (query tile, chunk) waves
// over the 256 CUs, chunks of at least 512 candidates so that the merge
// stays a small fraction of the scoring, rounded up to whole 16-item tiles.
extern "C" long long fma_topk_chunk_items(long long nq, long long nc,
                                          int topk) {
    if (!topk_shape_ok(nq, nc, topk, 0)) return -1;
    const long long nqt = (nq + 15) / 16;
    long long want = 2048 / nqt;
    if (want < 1) want = 1;
    long long chunk = (nc + want - 1) / want;
    chunk = (chunk + 15) / 16 * 16;
    return chunk < 512 ? 512 : chunk;
}

extern "C" long long fma_topk_workspace_bytes(long long nq, long long nc,
                                              int topk,
                                              long long chunk_items) {
    if (!topk_shape_ok(nq, nc, topk, chunk_items)) return -1;
    const long long chunk =
        chunk_items > 0 ? chunk_items : fma_topk_chunk_items(nq, nc, topk);
    const long long nchunks = (nc + chunk - 1) / chunk;
    return nq * nchunks * topk * (long long)sizeof(u64);
}

template <int KB, int WPB>
static void topk_launch_partial(const unsigned short* Q,
                                const unsigned short* V,
                                const long long* cand,
                                const long long* excl_ptr,
                                const long long* excl_rows, u64* ws,
                                long long nq, long long nc, int k, int topk,
                                long long chunk, long long nchunks,
                                long long nqt, int vec, hipStream_t stream) {
    const long long units = nqt * nchunks;
    const unsigned grid = (unsigned)((units + WPB - 1) / WPB);
    k_topk_partial<KB, WPB><<<dim3(grid), dim3(WPB * 64), 0, stream>>>(
        Q, V, cand, excl_ptr, excl_rows, ws, nq, nc, k, topk, chunk, nchunks,
        nqt, vec);
}

extern "C" int fma_topk_scores(
    const unsigned short* Q, const unsigned short* V, const long long* cand,
    const long long* excl_ptr, const long long* excl_rows, float* out_scores,
    long long* out_rows, void* workspace, long long workspace_bytes,
    long long nq, long long nv, long long nc, int k, int topk,
    long long chunk_items, void* stream) {
    if (!topk_shape_ok(nq, nc, topk, chunk_items) || k < 1 || k > 128 ||
        nv < 1 || nv >= (1ll << 31) || (cand == nullptr && nc != nv))
        return hipErrorInvalidValue;
    const long long need =
        fma_topk_workspace_bytes(nq, nc, topk, chunk_items);
    if (workspace == nullptr || workspace_bytes < need ||
        ((size_t)workspace & 7u) != 0)
        return hipErrorInvalidValue;
    const long long chunk =
        chunk_items > 0 ? chunk_items : fma_topk_chunk_items(nq, nc, topk);
    const long long nchunks = (nc + chunk - 1) / chunk;
    const long long nqt = (nq + 15) / 16;
    if (nqt * nchunks > (1ll << 31)) return hipErrorInvalidValue;
    const int vec = k % 8 == 0 && ((size_t)Q & 15u) == 0 &&
                    ((size_t)V & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    u64* ws = (u64*)workspace;
#define TOPK_PARTIAL(KB, WPB)                                               \
    topk_launch_partial<KB, WPB>(Q, V, cand, excl_ptr, excl_rows, ws, nq,   \
                                 nc, k, topk, chunk, nchunks, nqt, vec, st)
    // LDS per block = WPB * 16 * 2 KB * 8 B: 16 / 32 / 64 / 64 KiB
    switch (topk_kb(topk)) {
    case 16: TOPK_PARTIAL(16, 4); break;
    case 32: TOPK_PARTIAL(32, 4); break;
    case 64: TOPK_PARTIAL(64, 4); break;
    default: TOPK_PARTIAL(128, 2); break;
    }
#undef TOPK_PARTIAL
    int err = hipGetLastError();
    if (err != 0) return err;
    k_topk_merge<<<dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st>>>(
        ws, out_scores, out_rows, nq, nchunks, topk);
    return hipGetLastError();
}

// ================================================================ K9
// Rank counts: for each (query, target) pair how many candidate rows score
// strictly above / equal to the target, on the high word of topk_key (the
// row plays no part: the tie-break is the caller's).  No reference analog.
//
//   k_rank_scan    one WAVE owns (16-pair tile) x (one candidate chunk).
//                  A fragments are Q[q_idx[p0 + (lane & 15)]]; the B
//                  fragments, topk_load_frag calls and MFMA step order are
//                  those of k_topk_partial, so a (query, row) score is the
//                  same 32 bits in both kernels.  A prelude runs the same
//                  steps against the tile's own 16 target vectors: pair i's
//                  target score is the diagonal element.  The scan keeps
//                  4 x 2 integer counters per lane -- no LDS, no lists, no
//                  exclusion search -- and writes one (greater, equal)
//                  partial per (pair, chunk).
//   k_rank_finish  one wave per pair sums the chunk partials and takes the
//                  pair's exclusion slice back out: it scores the excluded
//                  rows in 16-row tiles and subtracts those the scan counted.
//                  Subtraction is only correct because the score bits here
//                  are identical to the scan's: same fragments, same MFMA
//                  steps, the query replicated into all 16 A rows (an MFMA
//                  output element depends on its own A row and B column
//                  only).  The launcher's contract makes every excluded row
//                  a candidate, counted exactly once by the scan.
//
// All sums are integers: the result cannot depend on chunking or the grid.

DEV_INLINE unsigned rank_word(float s) {
    return (unsigned)(topk_key(s, 0u) >> 32);
}

DEV_INLINE long long rank_group_sum(unsigned x) {
    // over the 16 lanes that share lane >> 4
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return (long long)x;
}

template <int WPB>
__launch_bounds__(WPB * 64)
__global__ void k_rank_scan(const unsigned short* __restrict__ Q,
                            const unsigned short* __restrict__ V,
                            const unsigned short* __restrict__ T,
                            const long long* __restrict__ q_idx,
                            const long long* __restrict__ skip,
                            const long long* __restrict__ cand,
                            long long* __restrict__ ws,
                            float* __restrict__ score, long long np,
                            long long nq, long long nc, int k,
                            long long chunk, long long nchunks,
                            long long npt, int vec) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    const long long unit = (long long)blockIdx.x * WPB + wv;
    if (unit >= npt * nchunks) return;     // waves are independent
    const long long pt = unit % npt, ch = unit / npt;
    const long long p0 = pt * 16;
    const long long cstart = ch * chunk;
    const long long cend = cstart + chunk < nc ? cstart + chunk : nc;
    const int KS = (k + 31) >> 5;

    // A fragments: Q[q_idx[p0 + li]][32 s + 8 g + 0..7], resident
    bf16x8 qf[4];
    {
        const unsigned short* qrow = nullptr;
        if (p0 + li < np) {
            const long long qi = q_idx[p0 + li];
            if (qi >= 0 && qi < nq) qrow = Q + qi * (long long)k;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[s] = topk_load_frag(s < KS ? qrow : nullptr, k, 32 * s + 8 * g,
                                   vec);
    }

    // prelude: the tile's 16 targets as B; lane li == 4 g + j holds pair
    // 4 g + j's target score in acc[j]
    unsigned tw[4];
    long long sk[4];
    {
        const unsigned short* trow =
            p0 + li < np ? T + (p0 + li) * (long long)k : nullptr;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < KS)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    qf[s],
                    topk_load_frag(trow, k, 32 * s + 8 * g, vec), acc, 0, 0,
                    0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = p0 + 4 * g + j;
            if (ch == 0 && li == 4 * g + j && p < np) score[p] = acc[j];
            tw[j] = rank_word(__shfl(acc[j], 20 * g + j, WAVE));
            sk[j] = p < np ? skip[p] : -1;
        }
    }

    unsigned gt[4] = {0u, 0u, 0u, 0u}, eq[4] = {0u, 0u, 0u, 0u};

    auto load_tile = [&](long long base, long long& r, bf16x8 (&vf)[4]) {
        const long long idx = base + li;
        r = -1;
        if (idx < cend) r = cand != nullptr ? cand[idx] : idx;
        const unsigned short* vrow = r >= 0 ? V + r * (long long)k : nullptr;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            vf[s] = topk_load_frag(s < KS ? vrow : nullptr, k,
                                   32 * s + 8 * g, vec);
    };

    long long r_cur;
    bf16x8 vf[4];
    load_tile(cstart, r_cur, vf);
    for (long long base = cstart; base < cend; base += 16) {
        // the next tile's loads fly while this one is scored and counted
        long long r_nxt = -1;
        bf16x8 vn[4];
        load_tile(base + 16, r_nxt, vn);

        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < KS)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], vf[s],
                                                              acc, 0, 0, 0);
        const bool live = r_cur >= 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned w = rank_word(acc[j]);
            // a strict "greater" can never hit the target itself
            gt[j] += (live && w > tw[j]) ? 1u : 0u;
            eq[j] += (live && w == tw[j] && r_cur != sk[j]) ? 1u : 0u;
        }
        r_cur = r_nxt;
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = vn[s];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long p = p0 + 4 * g + j;
        const long long sg = rank_group_sum(gt[j]);
        const long long se = rank_group_sum(eq[j]);
        if (li == 0 && p < np) {
            long long* dst = ws + (p * nchunks + ch) * 2;
            dst[0] = sg;
            dst[1] = se;
        }
    }
}

__launch_bounds__(256)
__global__ void k_rank_finish(const unsigned short* __restrict__ Q,
                              const unsigned short* __restrict__ V,
                              const long long* __restrict__ q_idx,
                              const long long* __restrict__ skip,
                              const long long* __restrict__ excl_ptr,
                              const long long* __restrict__ excl_rows,
                              const long long* __restrict__ ws,
                              const float* __restrict__ score,
                              long long* __restrict__ greater,
                              long long* __restrict__ equal, long long np,
                              long long nq, long long nv, int k,
                              long long nchunks, int vec) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = lane >> 4, li = lane & 15;
    const long long p = (long long)blockIdx.x * 4 + wv;
    if (p >= np) return;
    const int KS = (k + 31) >> 5;

    long long sg = 0, se = 0;
    for (long long c = lane; c < nchunks; c += 64) {
        sg += ws[(p * nchunks + c) * 2];
        se += ws[(p * nchunks + c) * 2 + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sg += __shfl_xor(sg, off, WAVE);
        se += __shfl_xor(se, off, WAVE);
    }

    const long long qi = q_idx[p];
    const bool qok = qi >= 0 && qi < nq;
    long long lo = 0, hi = 0;
    if (excl_ptr != nullptr && qok) {
        lo = excl_ptr[qi];
        hi = excl_ptr[qi + 1];
    }
    if (lo < hi) {                         // wave-uniform
        // the query in every A row: each lane's acc[0] is the score of the
        // tile's row li, the same bits k_rank_scan compared
        const unsigned short* qrow = Q + qi * (long long)k;
        bf16x8 qf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            qf[s] = topk_load_frag(s < KS ? qrow : nullptr, k, 32 * s + 8 * g,
                                   vec);
        const unsigned tw = rank_word(score[p]);
        const long long sk = skip[p];
        unsigned xg = 0u, xe = 0u;
        for (long long base = lo; base < hi; base += 16) {
            long long r = -1;
            if (base + li < hi) r = excl_rows[base + li];
            if (r >= nv) r = -1;           // never read past V
            const unsigned short* vrow =
                r >= 0 ? V + r * (long long)k : nullptr;
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (s < KS)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        qf[s],
                        topk_load_frag(vrow, k, 32 * s + 8 * g, vec), acc, 0,
                        0, 0);
            const unsigned w = rank_word(acc[0]);
            const bool counted = r >= 0 && r != sk;
            xg += (counted && w > tw) ? 1u : 0u;
            xe += (counted && w == tw) ? 1u : 0u;
        }
        // the four lane groups hold the same counts
        sg -= rank_group_sum(xg);
        se -= rank_group_sum(xe);
    }
    if (lane == 0) {
        greater[p] = sg;
        equal[p] = se;
    }
}

static bool rank_shape_ok(long long np, long long nc, long long chunk_items) {
    return np >= 1 && nc >= 1 && nc < (1ll << 31) && chunk_items >= 0;
}

// Chunk length the launcher picks: about 2048 (pair tile, chunk) waves over
// the 256 CUs, chunks of at least 512 candidates, whole 16-item tiles.
extern "C" long long fma_rank_chunk_items(long long np, long long nc) {
    if (!rank_shape_ok(np, nc, 0)) return -1;
    const long long npt = (np + 15) / 16;
    long long want = 2048 / npt;
    if (want < 1) want = 1;
    long long chunk = (nc + want - 1) / want;
    chunk = (chunk + 15) / 16 * 16;
    return chunk < 512 ? 512 : chunk;
}

extern "C" long long fma_rank_workspace_bytes(long long np, long long nc,
                                              long long chunk_items) {
    if (!rank_shape_ok(np, nc, chunk_items)) return -1;
    const long long chunk =
        chunk_items > 0 ? chunk_items : fma_rank_chunk_items(np, nc);
    const long long nchunks = (nc + chunk - 1) / chunk;
    return np * nchunks * 2 * (long long)sizeof(long long);
}

extern "C" int fma_rank_counts(
    const unsigned short* Q, const unsigned short* V, const unsigned short* T,
    const long long* q_idx, const long long* skip, const long long* cand,
    const long long* excl_ptr, const long long* excl_rows,
    long long* greater, long long* equal, float* score, void* workspace,
    long long workspace_bytes, long long np, long long nq, long long nv,
    long long nc, int k, long long chunk_items, void* stream) {
    if (!rank_shape_ok(np, nc, chunk_items) || k < 1 || k > 128 || nq < 1 ||
        nv < 1 || nv >= (1ll << 31) || (cand == nullptr && nc != nv) ||
        (excl_ptr != nullptr && excl_rows == nullptr))
        return hipErrorInvalidValue;
    const long long need = fma_rank_workspace_bytes(np, nc, chunk_items);
    if (workspace == nullptr || workspace_bytes < need ||
        ((size_t)workspace & 7u) != 0)
        return hipErrorInvalidValue;
    const long long chunk =
        chunk_items > 0 ? chunk_items : fma_rank_chunk_items(np, nc);
    const long long nchunks = (nc + chunk - 1) / chunk;
    const long long npt = (np + 15) / 16;
    if (npt * nchunks > (1ll << 31) || np > (1ll << 32))
        return hipErrorInvalidValue;
    const int vec = k % 8 == 0 && ((size_t)Q & 15u) == 0 &&
                    ((size_t)V & 15u) == 0 && ((size_t)T & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    constexpr int WPB = 4;
    const long long units = npt * nchunks;
    k_rank_scan<WPB><<<dim3((unsigned)((units + WPB - 1) / WPB)),
                       dim3(WPB * 64), 0, st>>>(
        Q, V, T, q_idx, skip, cand, (long long*)workspace, score, np, nq, nc,
        k, chunk, nchunks, npt, vec);
    int err = hipGetLastError();
    if (err != 0) return err;
    k_rank_finish<<<dim3((unsigned)((np + 3) / 4)), dim3(256), 0, st>>>(
        Q, V, q_idx, skip, excl_ptr, excl_rows, (const long long*)workspace,
        score, greater, equal, np, nq, nv, k, nchunks, vec);
    return hipGetLastError();
}
