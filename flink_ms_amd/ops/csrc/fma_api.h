// The C ABI between the HIP translation units and bindings.cpp, declared
// once.  The .hip files include this header and DEFINE every entry point
// with exactly these signatures (a drifted argument list fails to compile
// there); bindings.cpp includes it and calls them.  Deliberately free of
// HIP and torch headers so both sides can see it:
//   status   int     (a hipError_t value; 0 = success, fma_err_str names it)
//   stream   void*   (a hipStream_t)
//   bf16     unsigned short words, e4m3 unsigned char bytes
//   int64    long long
// Optional pointers (row_order, the low-precision output images, perm,
// err_out) may be null.  Launchers validate k and nrows only; everything
// about the tensors behind the pointers is the binding's job.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

const char* fma_err_str(int err);

// ---- ALS, block path (k = 16..128): als_kernels.hip
// fp8 != 0: factors are e4m3 bytes and the low-precision image written is
// out_fp8; else bf16 words and out_bf16.  The other image must be null.
int fma_als_solve_fused(int k, int fp8, const long long* indptr,
                        const int* indices, const float* values,
                        const void* factors, float* out_f32,
                        unsigned short* out_bf16, unsigned char* out_fp8,
                        const int* row_order, long long nrows, float reg,
                        void* stream);
int fma_gramian(int k, int fp8, const long long* indptr, const int* indices,
                const float* values, const void* factors, float* A_out,
                float* b_out, const int* row_order, long long nrows,
                float reg, void* stream);
// phases bitmask: 1 = eliminate, 2 = substitute
int fma_cholesky_solve_ph(int k, const float* A_in, const float* b_in,
                          float* x_out, long long nrows, int phases,
                          void* stream);
int fma_cholesky_solve(int k, const float* A_in, const float* b_in,
                       float* x_out, long long nrows, void* stream);

// ---- ALS, wave path (k = 16..64).  variant: a WREG_BC_* broadcast level
// (0..3; the _reg and _db kernels exist for 0 and 3 only)
int fma_ldl_solve_wave(int k, const float* A_in, const float* b_in,
                       float* x_out, unsigned short* x_bf16,
                       unsigned char* x_fp8, long long nrows, void* stream);
int fma_ldl_solve_wave_reg(int k, const float* A_in, const float* b_in,
                           float* x_out, unsigned short* x_bf16,
                           unsigned char* x_fp8, long long nrows, int variant,
                           void* stream);
int fma_als_solve_wavefused(int k, int fp8, const long long* indptr,
                            const int* indices, const float* values,
                            const void* factors, float* out_f32,
                            unsigned short* out_bf16, unsigned char* out_fp8,
                            const int* row_order, long long nrows, float reg,
                            int variant, void* stream);
// e4m3 factors only
int fma_als_solve_wavefused_db(int k, const long long* indptr,
                               const int* indices, const float* values,
                               const void* factors, float* out_f32,
                               unsigned short* out_bf16,
                               unsigned char* out_fp8, const int* row_order,
                               long long nrows, float reg, int variant,
                               void* stream);

// ---- ALS, weighted normal equations (implicit feedback): als_kernels.hip
// The twins of fma_gramian / fma_als_solve_fused / fma_als_solve_wavefused
// with, per stored entry j, scale[j] and ext[j] (fp32, the length of
// indices) in place of values, and the symmetric fp32 base matrix
// base[k][k] (only its lower triangle is read):
//   row~_j = round_D(scale[j] * dequant(factors[indices[j]]))
//   A = base + sum_j row~_j row~_j^T + reg * n * I,  b = sum_j ext[j] row~_j
// (ext through the same hi/lo pair as the explicit kernels' ratings).  All
// three pointers are required.  The wave-fused twin has the default
// broadcast level only.
int fma_gramian_w(int k, int fp8, const long long* indptr, const int* indices,
                  const float* scale, const float* ext, const float* base,
                  const void* factors, float* A_out, float* b_out,
                  const int* row_order, long long nrows, float reg,
                  void* stream);
int fma_als_solve_fused_w(int k, int fp8, const long long* indptr,
                          const int* indices, const float* scale,
                          const float* ext, const float* base,
                          const void* factors, float* out_f32,
                          unsigned short* out_bf16, unsigned char* out_fp8,
                          const int* row_order, long long nrows, float reg,
                          void* stream);
int fma_als_solve_wavefused_w(int k, int fp8, const long long* indptr,
                              const int* indices, const float* scale,
                              const float* ext, const float* base,
                              const void* factors, float* out_f32,
                              unsigned short* out_bf16,
                              unsigned char* out_fp8, const int* row_order,
                              long long nrows, float reg, void* stream);

// G [k][k] fp32 = sum over the n rows of the bf16 / e4m3 table factors
// [n][k] of f f^T, full and exactly symmetric, k = 16..128.  Parts of
// rows_per_part rows (0 = fma_factor_gram_rows_per_part; else rounded up to
// a multiple of 32) are accumulated by one wave each into workspace
// (fma_factor_gram_workspace_bytes, 4-byte aligned) and summed in part
// order: bit-reproducible, no atomics.  The size helpers return -1 for a
// bad shape (n < 1, k not a multiple of 16 in 16..128).
int fma_factor_gram(int k, int fp8, const void* factors, long long n,
                    long long rows_per_part, float* G, void* workspace,
                    long long workspace_bytes, void* stream);
// The same over a row list: G = sum_j f[rows[j]] f[rows[j]]^T for the nlist
// int32 entries of rows, each a row of the [ntable][k] table (not checked;
// repeats count once per occurrence, any order).  Parts are over list
// positions; the workspace is fma_factor_gram_workspace_bytes(nlist, k,
// rows_per_part).  With the same rows_per_part, bit-equal to
// fma_factor_gram on the compacted table.
int fma_factor_gram_rows(int k, int fp8, const void* factors,
                         long long ntable, const int* rows, long long nlist,
                         long long rows_per_part, float* G, void* workspace,
                         long long workspace_bytes, void* stream);
long long fma_factor_gram_workspace_bytes(long long n, int k,
                                          long long rows_per_part);
long long fma_factor_gram_rows_per_part(long long n, int k);

// ---- MFMA layout probes: fixed-size operands (als_kernels.hip)
int fma_mfma_probe_f32(const float* A /*[16][4]*/, const float* B /*[4][16]*/,
                       float* D /*[16][16]*/, void* stream);
int fma_mfma_probe_bf16(const unsigned short* Xt /*[32][16]*/,
                        const unsigned short* Yt /*[32][16]*/,
                        float* C /*[16][16]*/, void* stream);
int fma_mfma_probe_fp8(const unsigned char* Xt /*[32][16]*/,
                       const unsigned char* Yt /*[32][16]*/,
                       float* C /*[16][16]*/, void* stream);

// ---- bring-up dumps of entity 0 / the split b columns: debug_kernels.hip
int fma_dbg_stage_dump(int k, const long long* indptr, const int* indices,
                       const float* values, const unsigned short* factors,
                       unsigned short* out /*[k+16][32]*/, void* stream);
int fma_dbg_stage_dump_fp8(int k, const long long* indptr, const int* indices,
                           const float* values, const unsigned char* factors,
                           unsigned char* out /*[k+16][32]*/, void* stream);
int fma_dbg_frag_dump(int k, const long long* indptr, const int* indices,
                      const float* values, const unsigned short* factors,
                      unsigned short* out /*[4][k/16+1][64][8]*/,
                      void* stream);
int fma_dbg_gramian(int k, const long long* indptr, const int* indices,
                    const float* values, const unsigned short* factors,
                    float* A_out, float* bhi_out, float* blo_out,
                    long long nrows, float reg, void* stream);

// ---- SVM: svm_kernels.hip
int fma_sdca_pass(const long long* indptr, const int* indices,
                  const float* values, const float* y, const float* norms_sq,
                  const int* perm, float* alpha, float* v, long long nrows,
                  float scale, void* stream);
long long fma_sdca_num_waves(long long nrows);
int fma_svm_margins(const long long* indptr, const int* indices,
                    const float* values, const float* w, float* out,
                    long long nrows, void* stream);

// ---- serving: serve_kernels.hip
int fma_predict_dot(const unsigned short* U, const unsigned short* V,
                    const long long* u_idx, const long long* i_idx,
                    float* out, long long nq, int k, void* stream);
int fma_sgd_update(unsigned short* U, unsigned short* V,
                   const long long* u_idx, const long long* i_idx,
                   const float* r, float* err_out, long long nq, int k,
                   float lr, float user_reg, float item_reg, void* stream);

// ---- top-N recommendations: topk_kernels.hip
// For each of the nq bf16 query rows of Q [nq][k]: the topk best of the nc
// candidate rows of V [nv][k] (cand, or null = rows 0..nv-1, then nc == nv)
// by fp32 dot, score descending and lower row of V first among equal
// scores; NaN scores last; short results padded with row -1 / score -inf.
// excl_ptr [nq+1] / excl_rows (both null = no exclusions): per query an
// ascending slice of rows of V that must not be returned.  chunk_items = 0
// lets the launcher choose (fma_topk_chunk_items); the result does not
// depend on it.  The launcher validates 1 <= k, topk <= 128, nq, nc >= 1,
// nv and nc < 2^31 and the workspace size (fma_topk_workspace_bytes, 8-byte
// aligned).  It reads V at every cand entry and excl_rows at every excl_ptr
// entry without a check: 0 <= cand < nv and 0 <= excl_ptr, non-decreasing,
// <= the length of excl_rows are the PYTHON WRAPPER's job (ops.topk_scores),
// not the binding's.  The two size helpers return -1 for a bad shape.
int fma_topk_scores(const unsigned short* Q, const unsigned short* V,
                    const long long* cand, const long long* excl_ptr,
                    const long long* excl_rows, float* out_scores,
                    long long* out_rows, void* workspace,
                    long long workspace_bytes, long long nq, long long nv,
                    long long nc, int k, int topk, long long chunk_items,
                    void* stream);
long long fma_topk_workspace_bytes(long long nq, long long nc, int topk,
                                   long long chunk_items);
long long fma_topk_chunk_items(long long nq, long long nc, int topk);

// ---- rank counts: topk_kernels.hip
// For each of the np pairs p, with query row Q[q_idx[p]] (Q bf16 [nq][k])
// and target VECTOR T[p] (T bf16 [np][k]): score[p] = their fp32 dot, and
// greater[p] / equal[p] = how many of the nc candidate rows of V [nv][k]
// (cand, or null = rows 0..nv-1, then nc == nv) score strictly above /
// equal to it, compared on the score word of the top-N key (NaN below -inf,
// -0 == +0; the row plays no part).  Not counted: the row skip[p] of V (-1
// = none; the target's own row when it lives in V) and the rows of the
// exclusion slice excl_rows[excl_ptr[q_idx[p]] .. excl_ptr[q_idx[p] + 1])
// (excl_ptr [nq+1], indexed by QUERY row; both null = no exclusions).
// Scores are the same 32 bits fma_topk_scores computes for (query, row).
// chunk_items = 0 lets the launcher choose (fma_rank_chunk_items); the
// result does not depend on it.  The launcher validates 1 <= k <= 128, np,
// nq, nc >= 1, nv and nc < 2^31 and the workspace (fma_rank_workspace_bytes
// = np * chunks * 16, 8-byte aligned).  The PYTHON WRAPPER (ops.rank_counts)
// owns the contents: 0 <= q_idx < nq, 0 <= cand < nv without repeats, and
// excl_ptr non-decreasing offsets into excl_rows whose slices hold each row
// at most once, every one of them a candidate -- the exclusions are taken
// back out of the full count, so an excluded non-candidate or a repeated row
// would be subtracted without having been counted.  The two size helpers
// return -1 for a bad shape.
int fma_rank_counts(const unsigned short* Q, const unsigned short* V,
                    const unsigned short* T, const long long* q_idx,
                    const long long* skip, const long long* cand,
                    const long long* excl_ptr, const long long* excl_rows,
                    long long* greater, long long* equal, float* score,
                    void* workspace, long long workspace_bytes, long long np,
                    long long nq, long long nv, long long nc, int k,
                    long long chunk_items, void* stream);
long long fma_rank_workspace_bytes(long long np, long long nc,
                                   long long chunk_items);
long long fma_rank_chunk_items(long long np, long long nc);

#ifdef __cplusplus
}
#endif
