// Python bindings for the flink_ms_amd HIP kernels.
//
// This translation unit is deliberately HIP-header-free: kernels live in the
// .hip files behind the C launchers of fma_api.h (the one declaration both
// sides compile against), so only hipcc ever sees device code and this file
// only sees torch tensors.  The current HIP stream is passed in from Python
// (torch.cuda.current_stream().cuda_stream).
//
// Every binding validates ALL of its tensors through one Args object before
// it launches: the launchers take raw pointers, so a wrong device, dtype or
// shape here would be an out-of-bounds access on the GPU, not an exception.

#include <torch/extension.h>

#include <charconv>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fma_api.h"

namespace {

// ---------------------------------------------------------------- ingest
// Threaded parser for ALS model-row blocks ("<id>,<U|I>,<f;f;...>\n" x n):
// the native replacement for the reference's Kafka-consumer row decode
// (ALSKafkaConsumer.java:73-82).  One pass splits lines across threads;
// each thread strtoll/strtof-parses its share in place.  Returns
// (ids int64[n], kinds uint8[n] (0=U,1=I), factors fp32[n][k],
//  payload byte offsets int64[n], payload byte lengths int64[n], n_bad).
// Rows with a wrong factor count or malformed fields are marked kind=255
// and skipped by the caller's scalar fallback.
py::tuple parse_als_block(py::object text_o, int64_t k) {
    // raw CPython buffer protocol: accepts bytes AND mmap objects
    // (zero-copy parse of a disk-resident model file — the
    // larger-than-memory serving path)
    Py_buffer view;
    if (PyObject_GetBuffer(text_o.ptr(), &view, PyBUF_SIMPLE) != 0)
        throw py::error_already_set();
    char* base = (char*)view.buf;
    Py_ssize_t total = view.len;
    // line index (single pass; cheap relative to float parsing)
    std::vector<std::pair<int64_t, int64_t>> lines;
    int64_t start = 0;
    for (int64_t i = 0; i < total; ++i) {
        if (base[i] == '\n') {
            if (i > start) lines.emplace_back(start, i);
            start = i + 1;
        }
    }
    if (start < total) lines.emplace_back(start, total);
    const int64_t n = (int64_t)lines.size();
    auto ids = torch::empty({n}, torch::kInt64);
    auto kinds = torch::empty({n}, torch::kUInt8);
    auto facs = torch::empty({n, k}, torch::kFloat32);
    auto poffs = torch::empty({n}, torch::kInt64);
    auto plens = torch::empty({n}, torch::kInt64);
    int64_t* idp = ids.data_ptr<int64_t>();
    uint8_t* kp = kinds.data_ptr<uint8_t>();
    float* fp = facs.data_ptr<float>();
    int64_t* op = poffs.data_ptr<int64_t>();
    int64_t* lp = plens.data_ptr<int64_t>();
    std::atomic<int64_t> bad{0};
    const int nthreads = (int)std::min<int64_t>(
        std::max<int64_t>(1, n / 20000),
        (int64_t)std::thread::hardware_concurrency());
    auto work = [&](int64_t lo, int64_t hi) {
        int64_t my_bad = 0;
        for (int64_t r = lo; r < hi; ++r) {
            // std::from_chars everywhere: bounded by `end` (the input may
            // be an mmap with no trailing NUL) and faster than strtod
            const char* q = base + lines[r].first;
            const char* end = base + lines[r].second;
            kp[r] = 255;
            long long id;
            auto ir = std::from_chars(q, end, id, 10);
            if (ir.ec != std::errc() || ir.ptr >= end || *ir.ptr != ',') {
                ++my_bad;
                continue;
            }
            q = ir.ptr + 1;
            uint8_t kind;
            if (*q == 'U') kind = 0;
            else if (*q == 'I') kind = 1;
            else { ++my_bad; continue; }
            ++q;
            if (q >= end || *q != ',') { ++my_bad; continue; }
            ++q;
            op[r] = q - base;
            lp[r] = end - q;
            float* frow = fp + r * k;
            int64_t c = 0;
            bool ok = true;
            while (q < end && c < k) {
                // parse as double then narrow: float-subnormal payloads
                // (e.g. 4.9e-324) must flush like strtof, not reject
                double dv;
                auto fr = std::from_chars(q, end, dv,
                                          std::chars_format::general);
                if (fr.ec == std::errc::result_out_of_range) {
                    dv = 0.0;  // double-range underflow only
                } else if (fr.ec != std::errc()) {
                    ok = false;
                    break;
                }
                frow[c] = (float)dv;
                q = fr.ptr;
                ++c;
                if (q < end) {
                    if (*q == ';') ++q;
                    else { ok = false; break; }
                }
            }
            if (!ok || c != k || q < end) { ++my_bad; continue; }
            idp[r] = (int64_t)id;
            kp[r] = kind;
        }
        bad += my_bad;
    };
    if (nthreads <= 1) {
        work(0, n);
    } else {
        std::vector<std::thread> ts;
        const int64_t per = (n + nthreads - 1) / nthreads;
        for (int t = 0; t < nthreads; ++t)
            ts.emplace_back(work, t * per,
                            std::min<int64_t>(n, (t + 1) * per));
        for (auto& t : ts) t.join();
    }
    PyBuffer_Release(&view);
    return py::make_tuple(ids, kinds, facs, poffs, plens, (int64_t)bad);
}


void check_hip(int err, const char* what) {
    TORCH_CHECK(err == 0, what, " failed: ", fma_err_str(err));
}

constexpr auto kF32 = torch::kFloat32;
constexpr auto kBF16 = torch::kBFloat16;
constexpr auto kU8 = torch::kUInt8;   // e4m3 factor images travel as bytes
constexpr auto kI32 = torch::kInt32;
constexpr auto kI64 = torch::kInt64;

// Raw pointers for the launchers; the dtype was checked by Args.
float* f32(const torch::Tensor& t) { return (float*)t.data_ptr(); }
const int* i32(const torch::Tensor& t) { return (const int*)t.data_ptr(); }
const long long* i64(const torch::Tensor& t) {
    return (const long long*)t.data_ptr();
}
unsigned short* bf16(const torch::Tensor& t) {
    return (unsigned short*)t.data_ptr();
}
unsigned char* u8(const torch::Tensor& t) {
    return (unsigned char*)t.data_ptr();
}

// The argument checks of one binding call.  Each tensor goes through
// tensor() or optional() (dtype, contiguity) and the shape helpers: all of
// that reads tensor metadata only.  stream() -- the one way a binding gets
// the stream it must hand to its launcher -- then refuses unless every
// tensor seen is on the GPU.  Every message starts with the binding's name
// and names the argument.
class Args {
public:
    explicit Args(const char* fn) : fn_(fn) {}

    void tensor(const torch::Tensor& t, torch::ScalarType dt,
                const char* name) {
        TORCH_CHECK(t.scalar_type() == dt, fn_, ": ", name, " must be ", dt,
                    ", got ", t.scalar_type());
        TORCH_CHECK(t.is_contiguous(), fn_, ": ", name,
                    " must be contiguous");
        if (!t.is_cuda() && !off_gpu_) off_gpu_ = name;
    }

    // optional tensor: empty means absent (any dtype or device); present
    // means dt, contiguous, at least min_numel elements
    bool optional(const torch::Tensor& t, torch::ScalarType dt,
                  const char* name, int64_t min_numel) {
        if (t.numel() == 0) return false;
        tensor(t, dt, name);
        TORCH_CHECK(t.numel() >= min_numel, fn_, ": ", name,
                    " must be empty or have at least ", min_numel,
                    " elements, got ", t.numel());
        return true;
    }

    // CSR triple; returns nrows
    int64_t csr(const torch::Tensor& indptr, const torch::Tensor& indices,
                const torch::Tensor& values) {
        tensor(indptr, kI64, "indptr");
        tensor(indices, kI32, "indices");
        tensor(values, kF32, "values");
        TORCH_CHECK(indptr.dim() == 1 && indptr.numel() >= 1, fn_,
                    ": indptr must be 1-D with nrows + 1 elements");
        TORCH_CHECK(indices.dim() == 1 && values.dim() == 1 &&
                        indices.numel() == values.numel(),
                    fn_, ": indices and values must be 1-D of one length");
        return indptr.numel() - 1;
    }

    // gathered factor matrix [n][k], bf16 or (uint8) e4m3; returns k
    int factors(const torch::Tensor& t, bool fp8, const char* name) {
        tensor(t, fp8 ? kU8 : kBF16, name);
        TORCH_CHECK(t.dim() == 2, fn_, ": ", name, " must be 2-D");
        return rank(t.size(1), name);
    }

    // batched systems A [n][k][k]; returns k
    int systems(const torch::Tensor& A, const char* name) {
        tensor(A, kF32, name);
        TORCH_CHECK(A.dim() == 3 && A.size(1) == A.size(2), fn_, ": ", name,
                    " must be [n][k][k]");
        return rank(A.size(1), name);
    }

    // dt matrix with at least nrows rows and exactly k columns
    void rows(const torch::Tensor& t, torch::ScalarType dt, const char* name,
              int64_t nrows, int k) {
        tensor(t, dt, name);
        TORCH_CHECK(t.dim() == 2 && t.size(0) >= nrows && t.size(1) == k, fn_,
                    ": ", name, " must be [>= ", nrows, "][", k, "], got ",
                    t.sizes());
    }

    // fp32 [>= nrows][k][k] (the Gramian's A output)
    void square_rows(const torch::Tensor& t, const char* name, int64_t nrows,
                     int k) {
        tensor(t, kF32, name);
        TORCH_CHECK(t.dim() == 3 && t.size(0) >= nrows && t.size(1) == k &&
                        t.size(2) == k,
                    fn_, ": ", name, " must be [>= ", nrows, "][", k, "][", k,
                    "], got ", t.sizes());
    }

    // flat buffer of exactly / at least n elements
    void flat(const torch::Tensor& t, torch::ScalarType dt, const char* name,
              int64_t n, bool exact) {
        tensor(t, dt, name);
        TORCH_CHECK(exact ? t.numel() == n : t.numel() >= n, fn_, ": ", name,
                    " must have ", exact ? "" : "at least ", n,
                    " elements, got ", t.numel());
    }

    // CSR pattern without values (the weighted kernels take scale / ext
    // instead); returns nrows
    int64_t csr_pattern(const torch::Tensor& indptr,
                        const torch::Tensor& indices) {
        tensor(indptr, kI64, "indptr");
        tensor(indices, kI32, "indices");
        TORCH_CHECK(indptr.dim() == 1 && indptr.numel() >= 1, fn_,
                    ": indptr must be 1-D with nrows + 1 elements");
        TORCH_CHECK(indices.dim() == 1, fn_, ": indices must be 1-D");
        return indptr.numel() - 1;
    }

    // weighted normal equations: scale / ext fp32, 1-D, one per stored
    // entry; base contiguous fp32 [k][k]
    void weights(const torch::Tensor& scale, const torch::Tensor& ext,
                 const torch::Tensor& base, const torch::Tensor& indices,
                 int k) {
        const torch::Tensor* per_entry[2] = {&scale, &ext};
        const char* names[2] = {"scale", "ext"};
        for (int i = 0; i < 2; ++i) {
            tensor(*per_entry[i], kF32, names[i]);
            TORCH_CHECK(per_entry[i]->dim() == 1 &&
                            per_entry[i]->numel() == indices.numel(),
                        fn_, ": ", names[i], " must be 1-D with one element "
                        "per stored entry (", indices.numel(), "), got ",
                        per_entry[i]->sizes());
        }
        tensor(base, kF32, "base");
        TORCH_CHECK(base.dim() == 2 && base.size(0) == k && base.size(1) == k,
                    fn_, ": base must be [", k, "][", k, "], got ",
                    base.sizes());
    }

    // optional launch schedule: empty, or int32 of length nrows
    const int* row_order(const torch::Tensor& t, int64_t nrows,
                         const char* name = "row_order") {
        if (t.numel() == 0) return nullptr;
        tensor(t, kI32, name);
        TORCH_CHECK(t.dim() == 1 && t.numel() == nrows, fn_, ": ", name,
                    " must be empty or 1-D with nrows = ", nrows,
                    " elements, got ", t.numel());
        return i32(t);
    }

    void* stream(int64_t s) const {
        TORCH_CHECK(!off_gpu_, fn_, ": ", off_gpu_ ? off_gpu_ : "",
                    " must be on the GPU");
        return (void*)s;
    }

    const char* name() const { return fn_; }

private:
    int rank(int64_t k, const char* name) {
        TORCH_CHECK(k > 0 && k % 16 == 0, fn_, ": ", name, " has rank ", k,
                    ", need a multiple of 16");
        return (int)k;
    }

    const char* fn_;
    const char* off_gpu_ = nullptr;   // first tensor seen off the GPU
};

// The low-precision images written beside an fp32 [rows][k] output: each
// empty, or typed and at least as large as that output.
struct LowpOut {
    unsigned short* bf16p = nullptr;
    unsigned char* fp8p = nullptr;
    LowpOut(Args& a, const torch::Tensor& out_f32,
            const torch::Tensor& out_bf16, const char* bf16_name,
            const torch::Tensor& out_fp8, const char* fp8_name) {
        if (a.optional(out_bf16, kBF16, bf16_name, out_f32.numel()))
            bf16p = bf16(out_bf16);
        if (a.optional(out_fp8, kU8, fp8_name, out_f32.numel()))
            fp8p = u8(out_fp8);
    }
};

// ------------------------------------------------------------------- ALS

// Lane-broadcast variant of the register LDL (WREG_BC_* in
// als_kernels.hip): 0 = the __shfl path kept as the measured baseline,
// 3 = readlane broadcasts + branch-free substitutions (the default), 1 and
// 2 = the intermediate ladder steps (k_als_solve_wavefused only).  Every
// variant computes bit-identical results; ``variant`` is the last, optional
// argument of the bindings that take one.
constexpr int64_t kBroadcastShfl = 0;
constexpr int64_t kBroadcastDefault = 3;

// block-fused path (k <= 128).  The factors' dtype selects bf16 vs e4m3
// gathers and, with it, the one low-precision image the kernel writes.
void als_solve_fused(torch::Tensor indptr, torch::Tensor indices,
                     torch::Tensor values, torch::Tensor factors,
                     torch::Tensor out_f32, torch::Tensor out_bf16,
                     torch::Tensor out_fp8, torch::Tensor row_order,
                     double reg, int64_t stream) {
    Args a("als_solve_fused");
    const int64_t nrows = a.csr(indptr, indices, values);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    a.rows(out_f32, kF32, "out_f32", nrows, k);
    const LowpOut lp(a, out_f32, out_bf16, "out_bf16", out_fp8, "out_fp8");
    TORCH_CHECK(fp8 ? !lp.bf16p : !lp.fp8p, a.name(), ": ",
                fp8 ? "out_bf16 must be empty with e4m3 factors"
                    : "out_fp8 must be empty with bf16 factors");
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_als_solve_fused(k, fp8, i64(indptr), i32(indices),
                                  f32(values), factors.data_ptr(),
                                  f32(out_f32), lp.bf16p, lp.fp8p, order,
                                  nrows, (float)reg, a.stream(stream)),
              a.name());
}

void gramian(torch::Tensor indptr, torch::Tensor indices, torch::Tensor values,
             torch::Tensor factors, torch::Tensor A_out, torch::Tensor b_out,
             torch::Tensor row_order, double reg, int64_t stream) {
    Args a("gramian");
    const int64_t nrows = a.csr(indptr, indices, values);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    a.square_rows(A_out, "A_out", nrows, k);
    a.rows(b_out, kF32, "b_out", nrows, k);
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_gramian(k, fp8, i64(indptr), i32(indices), f32(values),
                          factors.data_ptr(), f32(A_out), f32(b_out), order,
                          nrows, (float)reg, a.stream(stream)),
              a.name());
}

// single-kernel k<=64 path: Gramian + register LDL in one wave per entity
// (no A materialization in HBM).  factors dtype selects bf16 vs e4m3.
void als_solve_wavefused(torch::Tensor indptr, torch::Tensor indices,
                         torch::Tensor values, torch::Tensor factors,
                         torch::Tensor out_f32, torch::Tensor out_bf16,
                         torch::Tensor out_fp8, torch::Tensor row_order,
                         double reg, int64_t stream, int64_t variant) {
    Args a("als_solve_wavefused");
    const int64_t nrows = a.csr(indptr, indices, values);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    a.rows(out_f32, kF32, "out_f32", nrows, k);
    const LowpOut lp(a, out_f32, out_bf16, "out_bf16", out_fp8, "out_fp8");
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_als_solve_wavefused(
                  k, fp8, i64(indptr), i32(indices), f32(values),
                  factors.data_ptr(), f32(out_f32), lp.bf16p, lp.fp8p, order,
                  nrows, (float)reg, (int)variant, a.stream(stream)),
              a.name());
}

// double-buffered variant (e4m3 only): software-pipelined staging
void als_solve_wavefused_db(torch::Tensor indptr, torch::Tensor indices,
                            torch::Tensor values, torch::Tensor factors,
                            torch::Tensor out_f32, torch::Tensor out_bf16,
                            torch::Tensor out_fp8, torch::Tensor row_order,
                            double reg, int64_t stream, int64_t variant) {
    Args a("als_solve_wavefused_db");
    const int64_t nrows = a.csr(indptr, indices, values);
    const int k = a.factors(factors, /*fp8=*/true, "factors");
    a.rows(out_f32, kF32, "out_f32", nrows, k);
    const LowpOut lp(a, out_f32, out_bf16, "out_bf16", out_fp8, "out_fp8");
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_als_solve_wavefused_db(
                  k, i64(indptr), i32(indices), f32(values),
                  factors.data_ptr(), f32(out_f32), lp.bf16p, lp.fp8p, order,
                  nrows, (float)reg, (int)variant, a.stream(stream)),
              a.name());
}

// ---- weighted normal equations (implicit feedback): the twins of
// gramian / als_solve_fused / als_solve_wavefused with (scale, ext, base)
// in place of values (fma_api.h has the contract)

void gramian_w(torch::Tensor indptr, torch::Tensor indices,
               torch::Tensor scale, torch::Tensor ext, torch::Tensor base,
               torch::Tensor factors, torch::Tensor A_out,
               torch::Tensor b_out, torch::Tensor row_order, double reg,
               int64_t stream) {
    Args a("gramian_w");
    const int64_t nrows = a.csr_pattern(indptr, indices);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    a.weights(scale, ext, base, indices, k);
    a.square_rows(A_out, "A_out", nrows, k);
    a.rows(b_out, kF32, "b_out", nrows, k);
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_gramian_w(k, fp8, i64(indptr), i32(indices), f32(scale),
                            f32(ext), f32(base), factors.data_ptr(),
                            f32(A_out), f32(b_out), order, nrows, (float)reg,
                            a.stream(stream)),
              a.name());
}

void als_solve_fused_w(torch::Tensor indptr, torch::Tensor indices,
                       torch::Tensor scale, torch::Tensor ext,
                       torch::Tensor base, torch::Tensor factors,
                       torch::Tensor out_f32, torch::Tensor out_bf16,
                       torch::Tensor out_fp8, torch::Tensor row_order,
                       double reg, int64_t stream) {
    Args a("als_solve_fused_w");
    const int64_t nrows = a.csr_pattern(indptr, indices);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    a.weights(scale, ext, base, indices, k);
    a.rows(out_f32, kF32, "out_f32", nrows, k);
    const LowpOut lp(a, out_f32, out_bf16, "out_bf16", out_fp8, "out_fp8");
    TORCH_CHECK(fp8 ? !lp.bf16p : !lp.fp8p, a.name(), ": ",
                fp8 ? "out_bf16 must be empty with e4m3 factors"
                    : "out_fp8 must be empty with bf16 factors");
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_als_solve_fused_w(
                  k, fp8, i64(indptr), i32(indices), f32(scale), f32(ext),
                  f32(base), factors.data_ptr(), f32(out_f32), lp.bf16p,
                  lp.fp8p, order, nrows, (float)reg, a.stream(stream)),
              a.name());
}

void als_solve_wavefused_w(torch::Tensor indptr, torch::Tensor indices,
                           torch::Tensor scale, torch::Tensor ext,
                           torch::Tensor base, torch::Tensor factors,
                           torch::Tensor out_f32, torch::Tensor out_bf16,
                           torch::Tensor out_fp8, torch::Tensor row_order,
                           double reg, int64_t stream) {
    Args a("als_solve_wavefused_w");
    const int64_t nrows = a.csr_pattern(indptr, indices);
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    TORCH_CHECK(k <= 64, a.name(), ": factors has rank ", k,
                ", the wave-fused kernel handles at most 64");
    a.weights(scale, ext, base, indices, k);
    a.rows(out_f32, kF32, "out_f32", nrows, k);
    const LowpOut lp(a, out_f32, out_bf16, "out_bf16", out_fp8, "out_fp8");
    const int* order = a.row_order(row_order, nrows);
    check_hip(fma_als_solve_wavefused_w(
                  k, fp8, i64(indptr), i32(indices), f32(scale), f32(ext),
                  f32(base), factors.data_ptr(), f32(out_f32), lp.bf16p,
                  lp.fp8p, order, nrows, (float)reg, a.stream(stream)),
              a.name());
}

// G [k][k] = F^T F of a bf16 / e4m3 table F [n][k], k = 16..128;
// rows_per_part = 0 is the launcher's choice
torch::Tensor factor_gram(torch::Tensor factors, int64_t rows_per_part,
                          int64_t stream) {
    Args a("factor_gram");
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    const int64_t n = factors.size(0);
    TORCH_CHECK(n >= 1, a.name(), ": factors must have at least one row");
    TORCH_CHECK(k <= 128, a.name(), ": factors has rank ", k,
                ", need at most 128");
    TORCH_CHECK(rows_per_part >= 0, a.name(),
                ": rows_per_part must be >= 0 (0 = the launcher's choice)");
    void* st = a.stream(stream);   // device check, before any allocation
    const long long ws_bytes =
        fma_factor_gram_workspace_bytes(n, k, rows_per_part);
    TORCH_CHECK(ws_bytes >= 0, a.name(), ": bad shape");
    auto opts = factors.options().dtype(kF32);
    auto ws = torch::empty({ws_bytes / 4}, opts);
    auto G = torch::empty({k, k}, opts);
    check_hip(fma_factor_gram(k, fp8, factors.data_ptr(), n, rows_per_part,
                              f32(G), ws.data_ptr(), ws_bytes, st),
              a.name());
    return G;
}

// G [k][k] = sum_j F[rows[j]] F[rows[j]]^T over an int32 row list of a
// bf16 / e4m3 table F [n][k], k = 16..128.  Rows may repeat (counted once
// per occurrence) and come in any order; every entry must be in [0, n) --
// the Python wrapper checks, the kernel does not.  With the same
// rows_per_part the result is bit-equal to factor_gram(F[rows]).
torch::Tensor factor_gram_rows(torch::Tensor factors, torch::Tensor rows,
                               int64_t rows_per_part, int64_t stream) {
    Args a("factor_gram_rows");
    const bool fp8 = factors.scalar_type() == kU8;
    const int k = a.factors(factors, fp8, "factors");
    const int64_t n = factors.size(0);
    a.tensor(rows, kI32, "rows");
    TORCH_CHECK(rows.dim() == 1, a.name(), ": rows must be 1-D, got ",
                rows.sizes());
    const int64_t nlist = rows.numel();
    TORCH_CHECK(nlist >= 1, a.name(), ": rows must have at least one entry");
    TORCH_CHECK(n >= 1 && n <= 0x7fffffffLL, a.name(),
                ": factors must have 1..2^31-1 rows, got ", n);
    TORCH_CHECK(k <= 128, a.name(), ": factors has rank ", k,
                ", need at most 128");
    TORCH_CHECK(rows_per_part >= 0, a.name(),
                ": rows_per_part must be >= 0 (0 = the launcher's choice)");
    void* st = a.stream(stream);   // device check, before any allocation
    TORCH_CHECK(rows.device() == factors.device(), a.name(),
                ": rows must be on the device of factors (", factors.device(),
                "), got ", rows.device());
    const long long ws_bytes =
        fma_factor_gram_workspace_bytes(nlist, k, rows_per_part);
    TORCH_CHECK(ws_bytes >= 0, a.name(), ": bad shape");
    auto opts = factors.options().dtype(kF32);
    auto ws = torch::empty({ws_bytes / 4}, opts);
    auto G = torch::empty({k, k}, opts);
    check_hip(fma_factor_gram_rows(k, fp8, factors.data_ptr(), n, i32(rows),
                                   nlist, rows_per_part, f32(G),
                                   ws.data_ptr(), ws_bytes, st),
              a.name());
    return G;
}

// Rows per part factor_gram uses for rows_per_part = 0; host-only.
int64_t factor_gram_rows_per_part(int64_t n, int64_t k) {
    const long long r = fma_factor_gram_rows_per_part(n, (int)k);
    TORCH_CHECK(r > 0, "factor_gram_rows_per_part: need n >= 1 and k a "
                       "multiple of 16 in 16..128");
    return (int64_t)r;
}

// Batched solves A x = b from dense systems: A [n][k][k], b and x
// [>= n][k].  Returns (n, k) through the out-parameters.
void solve_args(Args& a, const torch::Tensor& A, const torch::Tensor& b,
                const torch::Tensor& x, int64_t& nrows, int& k) {
    k = a.systems(A, "A");
    nrows = A.size(0);
    a.rows(b, kF32, "b", nrows, k);
    a.rows(x, kF32, "x", nrows, k);
}

// phases bitmask (debug/ablation): 1 = eliminate, 2 = substitute
void cholesky_solve_ph(torch::Tensor A, torch::Tensor b, torch::Tensor x,
                       int64_t phases, int64_t stream) {
    Args a("cholesky_solve_ph");
    int64_t nrows;
    int k;
    solve_args(a, A, b, x, nrows, k);
    TORCH_CHECK(phases >= 0 && phases <= 3, a.name(),
                ": phases must be in 0..3, got ", phases);
    check_hip(fma_cholesky_solve_ph(k, f32(A), f32(b), f32(x), nrows,
                                    (int)phases, a.stream(stream)),
              a.name());
}

void cholesky_solve(torch::Tensor A, torch::Tensor b, torch::Tensor x,
                    int64_t stream) {
    Args a("cholesky_solve");
    int64_t nrows;
    int k;
    solve_args(a, A, b, x, nrows, k);
    check_hip(fma_cholesky_solve(k, f32(A), f32(b), f32(x), nrows,
                                 a.stream(stream)),
              a.name());
}

// wave-per-entity LDL over an LDS image (v1, k <= 64)
void ldl_solve_wave(torch::Tensor A, torch::Tensor b, torch::Tensor x,
                    torch::Tensor x_bf16, torch::Tensor x_fp8,
                    int64_t stream) {
    Args a("ldl_solve_wave");
    int64_t nrows;
    int k;
    solve_args(a, A, b, x, nrows, k);
    const LowpOut lp(a, x, x_bf16, "x_bf16", x_fp8, "x_fp8");
    check_hip(fma_ldl_solve_wave(k, f32(A), f32(b), f32(x), lp.bf16p, lp.fp8p,
                                 nrows, a.stream(stream)),
              a.name());
}

// register-resident v2 (A in MFMA fragments, panel scratch in LDS)
void ldl_solve_wave_reg(torch::Tensor A, torch::Tensor b, torch::Tensor x,
                        torch::Tensor x_bf16, torch::Tensor x_fp8,
                        int64_t stream, int64_t variant) {
    Args a("ldl_solve_wave_reg");
    int64_t nrows;
    int k;
    solve_args(a, A, b, x, nrows, k);
    const LowpOut lp(a, x, x_bf16, "x_bf16", x_fp8, "x_fp8");
    check_hip(fma_ldl_solve_wave_reg(k, f32(A), f32(b), f32(x), lp.bf16p,
                                     lp.fp8p, nrows, (int)variant,
                                     a.stream(stream)),
              a.name());
}

// ------------------------------------------------------------------- SVM

void sdca_pass(torch::Tensor indptr, torch::Tensor indices,
               torch::Tensor values, torch::Tensor y, torch::Tensor norms_sq,
               torch::Tensor perm, torch::Tensor alpha, torch::Tensor v,
               double scale, int64_t stream) {
    Args a("sdca_pass");
    // the kernel indexes all per-sample arrays by row id: sizes must agree
    // before anything is launched
    const int64_t nrows = a.csr(indptr, indices, values);
    a.flat(y, kF32, "y", nrows, /*exact=*/true);
    a.flat(norms_sq, kF32, "norms_sq", nrows, true);
    a.flat(alpha, kF32, "alpha", nrows, true);
    a.tensor(v, kF32, "v");
    const int* p = a.row_order(perm, nrows, "perm");
    check_hip(fma_sdca_pass(i64(indptr), i32(indices), f32(values), f32(y),
                            f32(norms_sq), p, f32(alpha), f32(v), nrows,
                            (float)scale, a.stream(stream)),
              a.name());
}

// Waves one sdca_pass launch over nrows samples runs with (the stride of the
// kernel's sample schedule); host-only, no GPU needed.
int64_t sdca_num_waves(int64_t nrows) {
    return (int64_t)fma_sdca_num_waves(nrows);
}

void svm_margins(torch::Tensor indptr, torch::Tensor indices,
                 torch::Tensor values, torch::Tensor w, torch::Tensor out,
                 int64_t stream) {
    Args a("svm_margins");
    const int64_t nrows = a.csr(indptr, indices, values);
    a.tensor(w, kF32, "w");
    a.flat(out, kF32, "out", nrows, /*exact=*/false);
    check_hip(fma_svm_margins(i64(indptr), i32(indices), f32(values), f32(w),
                              f32(out), nrows, a.stream(stream)),
              a.name());
}

// --------------------------------------------------------------- serving

// U, V bf16 [n][k] of one rank; u_idx, i_idx int64 of one length.  Returns
// the number of queries.
int64_t serve_args(Args& a, const torch::Tensor& U, const torch::Tensor& V,
                   const torch::Tensor& u_idx, const torch::Tensor& i_idx) {
    a.tensor(U, kBF16, "U");
    a.tensor(V, kBF16, "V");
    a.tensor(u_idx, kI64, "u_idx");
    TORCH_CHECK(U.dim() == 2 && V.dim() == 2, a.name(),
                ": U and V must be 2-D");
    TORCH_CHECK(U.size(1) == V.size(1), a.name(), ": U/V rank mismatch");
    a.flat(i_idx, kI64, "i_idx", u_idx.numel(), /*exact=*/true);
    return u_idx.numel();
}

void predict_dot(torch::Tensor U, torch::Tensor V, torch::Tensor u_idx,
                 torch::Tensor i_idx, torch::Tensor out, int64_t stream) {
    Args a("predict_dot");
    const int64_t nq = serve_args(a, U, V, u_idx, i_idx);
    a.flat(out, kF32, "out", nq, /*exact=*/false);
    check_hip(fma_predict_dot(bf16(U), bf16(V), i64(u_idx), i64(i_idx),
                              f32(out), nq, (int)U.size(1),
                              a.stream(stream)),
              a.name());
}

void sgd_update(torch::Tensor U, torch::Tensor V, torch::Tensor u_idx,
                torch::Tensor i_idx, torch::Tensor r, torch::Tensor err_out,
                double lr, double user_reg, double item_reg, int64_t stream) {
    Args a("sgd_update");
    const int64_t nq = serve_args(a, U, V, u_idx, i_idx);
    a.flat(r, kF32, "r", nq, /*exact=*/true);
    float* ep = a.optional(err_out, kF32, "err_out", nq) ? f32(err_out)
                                                         : nullptr;
    check_hip(fma_sgd_update(bf16(U), bf16(V), i64(u_idx), i64(i_idx), f32(r),
                             ep, nq, (int)U.size(1), (float)lr,
                             (float)user_reg, (float)item_reg,
                             a.stream(stream)),
              a.name());
}

// Top-N: Q bf16 [nq][k] queries against the cand rows (empty = all) of V
// bf16 [nv][k]; excl_ptr [nq+1] / excl_rows (both empty = none) are the
// per-query sorted exclusion slices.  Returns (scores fp32 [nq][topk],
// rows int64 [nq][topk]).  The CONTENTS of cand and excl_ptr index device
// memory and are range-checked by the Python wrapper (ops.topk_scores),
// which is the only caller; this binding checks metadata.
py::tuple topk_scores(torch::Tensor Q, torch::Tensor V, torch::Tensor cand,
                      torch::Tensor excl_ptr, torch::Tensor excl_rows,
                      int64_t topk, int64_t chunk_items, int64_t stream) {
    Args a("topk_scores");
    a.tensor(Q, kBF16, "Q");
    a.tensor(V, kBF16, "V");
    TORCH_CHECK(Q.dim() == 2 && V.dim() == 2, a.name(),
                ": Q and V must be 2-D");
    TORCH_CHECK(Q.size(1) == V.size(1), a.name(), ": Q/V rank mismatch");
    const int64_t nq = Q.size(0), nv = V.size(0), k = Q.size(1);
    TORCH_CHECK(nq >= 1 && nv >= 1, a.name(),
                ": Q and V must have at least one row");
    TORCH_CHECK(k >= 1 && k <= 128, a.name(), ": rank k = ", k,
                " must be in 1..128");
    TORCH_CHECK(topk >= 1 && topk <= 128, a.name(), ": topk = ", topk,
                " must be in 1..128");
    TORCH_CHECK(chunk_items >= 0, a.name(),
                ": chunk_items must be >= 0 (0 = the launcher's choice)");
    const long long* candp = nullptr;
    int64_t nc = nv;
    if (a.optional(cand, kI64, "cand", 1)) {
        TORCH_CHECK(cand.dim() == 1, a.name(), ": cand must be 1-D");
        candp = i64(cand);
        nc = cand.numel();
    }
    TORCH_CHECK(nv < (int64_t(1) << 31) && nc < (int64_t(1) << 31), a.name(),
                ": V and cand must have fewer than 2^31 rows");
    const long long* eptr = nullptr;
    const long long* erows = nullptr;
    if (a.optional(excl_ptr, kI64, "excl_ptr", 1)) {
        TORCH_CHECK(excl_ptr.dim() == 1 && excl_ptr.numel() == nq + 1,
                    a.name(), ": excl_ptr must be 1-D with nq + 1 = ", nq + 1,
                    " elements, got ", excl_ptr.numel());
        eptr = i64(excl_ptr);
        if (a.optional(excl_rows, kI64, "excl_rows", 1)) {
            TORCH_CHECK(excl_rows.dim() == 1, a.name(),
                        ": excl_rows must be 1-D");
            erows = i64(excl_rows);
        }
    } else {
        TORCH_CHECK(excl_rows.numel() == 0, a.name(),
                    ": excl_rows given without excl_ptr");
    }
    void* st = a.stream(stream);   // device check, before any allocation
    const long long ws_bytes =
        fma_topk_workspace_bytes(nq, nc, (int)topk, chunk_items);
    TORCH_CHECK(ws_bytes >= 0, a.name(), ": bad shape");
    auto opts = Q.options();
    auto ws = torch::empty({(ws_bytes + 7) / 8}, opts.dtype(kI64));
    auto scores = torch::empty({nq, topk}, opts.dtype(kF32));
    auto rows = torch::empty({nq, topk}, opts.dtype(kI64));
    check_hip(fma_topk_scores(bf16(Q), bf16(V), candp, eptr, erows,
                              f32(scores), (long long*)rows.data_ptr(),
                              ws.data_ptr(), ws_bytes, nq, nv, nc, (int)k,
                              (int)topk, chunk_items, st),
              a.name());
    return py::make_tuple(scores, rows);
}

// Chunk length topk_scores uses for chunk_items = 0; host-only.
int64_t topk_chunk_items(int64_t nq, int64_t nc, int64_t topk) {
    TORCH_CHECK(topk >= 1 && topk <= 128 && nq >= 1 && nc >= 1 &&
                    nc < (int64_t(1) << 31),
                "topk_chunk_items: need nq, nc >= 1, nc < 2^31 and topk in "
                "1..128");
    return (int64_t)fma_topk_chunk_items(nq, nc, (int)topk);
}

// Rank counts: for pair p the query Q[q_idx[p]] (Q bf16 [nq][k]) against the
// cand rows (empty = all) of V bf16 [nv][k], relative to the target VECTOR
// T[p] (T bf16 [P][k]); skip [P] is the row of V not to count (-1 = none);
// excl_ptr [nq+1] / excl_rows (both empty = none) are per-QUERY-ROW slices.
// Returns (greater int64 [P], equal int64 [P], score fp32 [P]).  The
// CONTENTS of q_idx, cand, excl_ptr and excl_rows index device memory and
// are checked by the Python wrapper (ops.rank_counts); this binding checks
// metadata.
py::tuple rank_counts(torch::Tensor Q, torch::Tensor V, torch::Tensor T,
                      torch::Tensor q_idx, torch::Tensor skip,
                      torch::Tensor cand, torch::Tensor excl_ptr,
                      torch::Tensor excl_rows, int64_t chunk_items,
                      int64_t stream) {
    Args a("rank_counts");
    a.tensor(Q, kBF16, "Q");
    a.tensor(V, kBF16, "V");
    a.tensor(T, kBF16, "T");
    TORCH_CHECK(Q.dim() == 2 && V.dim() == 2 && T.dim() == 2, a.name(),
                ": Q, V and T must be 2-D");
    TORCH_CHECK(Q.size(1) == V.size(1) && Q.size(1) == T.size(1), a.name(),
                ": Q/V/T rank mismatch");
    const int64_t nq = Q.size(0), nv = V.size(0), k = Q.size(1);
    const int64_t np = T.size(0);
    TORCH_CHECK(nq >= 1 && nv >= 1 && np >= 1, a.name(),
                ": Q, V and T must have at least one row");
    TORCH_CHECK(k >= 1 && k <= 128, a.name(), ": rank k = ", k,
                " must be in 1..128");
    TORCH_CHECK(chunk_items >= 0, a.name(),
                ": chunk_items must be >= 0 (0 = the launcher's choice)");
    a.tensor(q_idx, kI64, "q_idx");
    a.tensor(skip, kI64, "skip");
    TORCH_CHECK(q_idx.dim() == 1 && q_idx.numel() == np, a.name(),
                ": q_idx must be 1-D with P = ", np, " elements, got ",
                q_idx.numel());
    TORCH_CHECK(skip.dim() == 1 && skip.numel() == np, a.name(),
                ": skip must be 1-D with P = ", np, " elements, got ",
                skip.numel());
    const long long* candp = nullptr;
    int64_t nc = nv;
    if (a.optional(cand, kI64, "cand", 1)) {
        TORCH_CHECK(cand.dim() == 1, a.name(), ": cand must be 1-D");
        candp = i64(cand);
        nc = cand.numel();
    }
    TORCH_CHECK(nv < (int64_t(1) << 31) && nc < (int64_t(1) << 31), a.name(),
                ": V and cand must have fewer than 2^31 rows");
    const long long* eptr = nullptr;
    const long long* erows = nullptr;
    if (a.optional(excl_ptr, kI64, "excl_ptr", 1)) {
        TORCH_CHECK(excl_ptr.dim() == 1 && excl_ptr.numel() == nq + 1,
                    a.name(), ": excl_ptr must be 1-D with nq + 1 = ", nq + 1,
                    " elements, got ", excl_ptr.numel());
        // an all-empty exclusion is no exclusion: the launcher never gets an
        // excl_ptr without rows behind it
        if (a.optional(excl_rows, kI64, "excl_rows", 1)) {
            TORCH_CHECK(excl_rows.dim() == 1, a.name(),
                        ": excl_rows must be 1-D");
            eptr = i64(excl_ptr);
            erows = i64(excl_rows);
        }
    } else {
        TORCH_CHECK(excl_rows.numel() == 0, a.name(),
                    ": excl_rows given without excl_ptr");
    }
    void* st = a.stream(stream);   // device check, before any allocation
    const long long ws_bytes = fma_rank_workspace_bytes(np, nc, chunk_items);
    TORCH_CHECK(ws_bytes >= 0, a.name(), ": bad shape");
    auto opts = Q.options();
    auto ws = torch::empty({(ws_bytes + 7) / 8}, opts.dtype(kI64));
    auto greater = torch::empty({np}, opts.dtype(kI64));
    auto equal = torch::empty({np}, opts.dtype(kI64));
    auto score = torch::empty({np}, opts.dtype(kF32));
    check_hip(fma_rank_counts(bf16(Q), bf16(V), bf16(T), i64(q_idx),
                              i64(skip), candp, eptr, erows,
                              (long long*)greater.data_ptr(),
                              (long long*)equal.data_ptr(), f32(score),
                              ws.data_ptr(), ws_bytes, np, nq, nv, nc, (int)k,
                              chunk_items, st),
              a.name());
    return py::make_tuple(greater, equal, score);
}

// Chunk length rank_counts uses for chunk_items = 0, -1 for a bad shape
// (P or nc < 1, nc >= 2^31); host-only.
int64_t rank_chunk_items(int64_t np, int64_t nc) {
    return (int64_t)fma_rank_chunk_items(np, nc);
}

// ------------------------------------------------- MFMA probes and dumps

void mfma_probe_f32(torch::Tensor A, torch::Tensor B, torch::Tensor D,
                    int64_t stream) {
    Args a("mfma_probe_f32");
    a.flat(A, kF32, "A", 16 * 4, /*exact=*/true);
    a.flat(B, kF32, "B", 4 * 16, true);
    a.flat(D, kF32, "D", 16 * 16, true);
    check_hip(fma_mfma_probe_f32(f32(A), f32(B), f32(D), a.stream(stream)),
              a.name());
}

void mfma_probe_bf16(torch::Tensor Xt, torch::Tensor Yt, torch::Tensor C,
                     int64_t stream) {
    Args a("mfma_probe_bf16");
    a.flat(Xt, kBF16, "Xt", 32 * 16, /*exact=*/true);
    a.flat(Yt, kBF16, "Yt", 32 * 16, true);
    a.flat(C, kF32, "C", 16 * 16, true);
    check_hip(fma_mfma_probe_bf16(bf16(Xt), bf16(Yt), f32(C),
                                  a.stream(stream)),
              a.name());
}

void mfma_probe_fp8(torch::Tensor Xt, torch::Tensor Yt, torch::Tensor C,
                    int64_t stream) {
    Args a("mfma_probe_fp8");
    a.flat(Xt, kU8, "Xt", 32 * 16, /*exact=*/true);
    a.flat(Yt, kU8, "Yt", 32 * 16, true);
    a.flat(C, kF32, "C", 16 * 16, true);
    check_hip(fma_mfma_probe_fp8(u8(Xt), u8(Yt), f32(C), a.stream(stream)),
              a.name());
}

// The dumps read entity 0 of the CSR (so it needs one) through the bf16
// stage; ``out`` holds the [k+16][32] stage image.
void dbg_stage_dump(torch::Tensor indptr, torch::Tensor indices,
                    torch::Tensor values, torch::Tensor factors,
                    torch::Tensor out, int64_t stream) {
    Args a("dbg_stage_dump");
    TORCH_CHECK(a.csr(indptr, indices, values) >= 1, a.name(),
                ": indptr must hold at least one entity");
    const int k = a.factors(factors, /*fp8=*/false, "factors");
    a.flat(out, kBF16, "out", (int64_t)(k + 16) * 32, /*exact=*/false);
    check_hip(fma_dbg_stage_dump(k, i64(indptr), i32(indices), f32(values),
                                 bf16(factors), bf16(out), a.stream(stream)),
              a.name());
}

// The same through the e4m3 stage: byte factors, [k+16][32]-byte image.
void dbg_stage_dump_fp8(torch::Tensor indptr, torch::Tensor indices,
                        torch::Tensor values, torch::Tensor factors,
                        torch::Tensor out, int64_t stream) {
    Args a("dbg_stage_dump_fp8");
    TORCH_CHECK(a.csr(indptr, indices, values) >= 1, a.name(),
                ": indptr must hold at least one entity");
    const int k = a.factors(factors, /*fp8=*/true, "factors");
    a.flat(out, kU8, "out", (int64_t)(k + 16) * 32, /*exact=*/false);
    check_hip(fma_dbg_stage_dump_fp8(k, i64(indptr), i32(indices),
                                     f32(values), u8(factors), u8(out),
                                     a.stream(stream)),
              a.name());
}

// ``out`` holds [4 waves][k/16 + 1 tiles][64 lanes][8] fragment elements.
void dbg_frag_dump(torch::Tensor indptr, torch::Tensor indices,
                   torch::Tensor values, torch::Tensor factors,
                   torch::Tensor out, int64_t stream) {
    Args a("dbg_frag_dump");
    TORCH_CHECK(a.csr(indptr, indices, values) >= 1, a.name(),
                ": indptr must hold at least one entity");
    const int k = a.factors(factors, /*fp8=*/false, "factors");
    a.flat(out, kBF16, "out", (int64_t)4 * (k / 16 + 1) * 64 * 8,
           /*exact=*/false);
    check_hip(fma_dbg_frag_dump(k, i64(indptr), i32(indices), f32(values),
                                bf16(factors), bf16(out), a.stream(stream)),
              a.name());
}

void dbg_gramian(torch::Tensor indptr, torch::Tensor indices,
                 torch::Tensor values, torch::Tensor factors,
                 torch::Tensor A_out, torch::Tensor bhi, torch::Tensor blo,
                 double reg, int64_t stream) {
    Args a("dbg_gramian");
    const int64_t nrows = a.csr(indptr, indices, values);
    const int k = a.factors(factors, /*fp8=*/false, "factors");
    a.square_rows(A_out, "A_out", nrows, k);
    a.rows(bhi, kF32, "bhi", nrows, k);
    a.rows(blo, kF32, "blo", nrows, k);
    check_hip(fma_dbg_gramian(k, i64(indptr), i32(indices), f32(values),
                              bf16(factors), f32(A_out), f32(bhi), f32(blo),
                              nrows, (float)reg, a.stream(stream)),
              a.name());
}

}  // namespace

void register_kvserver(pybind11::module_& m);  // serving/csrc/kvserver.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "flink_ms_amd MI355X (gfx950) HIP kernels";
    register_kvserver(m);
    m.def("als_solve_fused", &als_solve_fused);
    m.def("gramian", &gramian);
    m.attr("BROADCAST_SHFL") = kBroadcastShfl;
    m.attr("BROADCAST_DEFAULT") = kBroadcastDefault;
    // ``variant`` is optional (positional or by name): BROADCAST_DEFAULT
    m.def("als_solve_wavefused", &als_solve_wavefused, py::arg("indptr"),
          py::arg("indices"), py::arg("values"), py::arg("factors"),
          py::arg("out_f32"), py::arg("out_bf16"), py::arg("out_fp8"),
          py::arg("row_order"), py::arg("reg"), py::arg("stream"),
          py::arg("variant") = kBroadcastDefault);
    m.def("als_solve_wavefused_db", &als_solve_wavefused_db,
          py::arg("indptr"), py::arg("indices"), py::arg("values"),
          py::arg("factors"), py::arg("out_f32"), py::arg("out_bf16"),
          py::arg("out_fp8"), py::arg("row_order"), py::arg("reg"),
          py::arg("stream"), py::arg("variant") = kBroadcastDefault);
    m.def("gramian_w", &gramian_w);
    m.def("als_solve_fused_w", &als_solve_fused_w);
    m.def("als_solve_wavefused_w", &als_solve_wavefused_w);
    m.def("factor_gram", &factor_gram, py::arg("factors"),
          py::arg("rows_per_part"), py::arg("stream"));
    m.def("factor_gram_rows", &factor_gram_rows, py::arg("factors"),
          py::arg("rows"), py::arg("rows_per_part"), py::arg("stream"));
    m.def("factor_gram_rows_per_part", &factor_gram_rows_per_part);
    m.def("cholesky_solve", &cholesky_solve);
    m.def("cholesky_solve_ph", &cholesky_solve_ph);
    m.def("ldl_solve_wave", &ldl_solve_wave);
    m.def("ldl_solve_wave_reg", &ldl_solve_wave_reg, py::arg("A"),
          py::arg("b"), py::arg("x"), py::arg("x_bf16"), py::arg("x_fp8"),
          py::arg("stream"), py::arg("variant") = kBroadcastDefault);
    m.def("sdca_pass", &sdca_pass);
    m.def("sdca_num_waves", &sdca_num_waves);
    m.def("svm_margins", &svm_margins);
    m.def("predict_dot", &predict_dot);
    m.def("sgd_update", &sgd_update);
    m.def("topk_scores", &topk_scores, py::arg("Q"), py::arg("V"),
          py::arg("cand"), py::arg("excl_ptr"), py::arg("excl_rows"),
          py::arg("topk"), py::arg("chunk_items"), py::arg("stream"));
    m.def("topk_chunk_items", &topk_chunk_items);
    m.def("rank_counts", &rank_counts, py::arg("Q"), py::arg("V"),
          py::arg("T"), py::arg("q_idx"), py::arg("skip"), py::arg("cand"),
          py::arg("excl_ptr"), py::arg("excl_rows"), py::arg("chunk_items"),
          py::arg("stream"));
    m.def("rank_chunk_items", &rank_chunk_items);
    m.def("dbg_stage_dump", &dbg_stage_dump);
    m.def("dbg_stage_dump_fp8", &dbg_stage_dump_fp8);
    m.def("dbg_frag_dump", &dbg_frag_dump);
    m.def("dbg_gramian", &dbg_gramian);
    m.def("mfma_probe_f32", &mfma_probe_f32);
    m.def("mfma_probe_bf16", &mfma_probe_bf16);
    m.def("mfma_probe_fp8", &mfma_probe_fp8);
    m.def("parse_als_block", &parse_als_block);
}
