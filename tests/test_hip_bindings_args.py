"""Argument validation at the extension boundary (bindings.cpp).

The launchers take raw pointers, so every binding has to reject a wrong
device, dtype, layout or shape before it launches.  The CPU part runs
wherever the extension is built (the checks read tensor metadata only and
the device check comes last, so shape errors are reachable without a GPU).
The GPU part feeds each binding arguments that are wrong in a way that could
not write out of bounds even if the check were missing (same-or-larger byte
size, never an undersized output), and verifies that nothing was written.
"""

import pytest
import torch

from flink_ms_amd import ops

if not ops.hip_available():
    pytest.skip("HIP extension not built", allow_module_level=True)

import flink_ms_amd._hip_ops as hip  # noqa: E402

K = 16
DEGREES = [0, 1, 3, 32, 33, 5, 2, 40]          # 8 entities, chunk edges
NROWS = len(DEGREES)
COLS = 50
SENTINEL = 12345.0


def _csr(device, degrees=DEGREES):
    g = torch.Generator().manual_seed(11)
    deg = torch.tensor(degrees)
    indptr = torch.zeros(len(degrees) + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    nnz = int(indptr[-1])
    indices = torch.randint(0, COLS, (nnz,), generator=g).to(torch.int32)
    values = torch.rand(nnz, generator=g) * 4.5 + 0.5
    return indptr.to(device), indices.to(device), values.to(device)


def _factors(device, fp8, k=K):
    f = torch.randn(COLS, k, generator=torch.Generator().manual_seed(k)) * 0.5
    return (ops.quantize_fp8(f) if fp8 else f.to(torch.bfloat16)).to(device)


def _outs(device, rows=NROWS, k=K):
    """Sentinel-filled fp32 / bf16 / e4m3 outputs."""
    return (torch.full((rows, k), SENTINEL, device=device),
            torch.full((rows, k), SENTINEL, device=device,
                       dtype=torch.bfloat16),
            torch.full((rows, k), 0x7F, device=device, dtype=torch.uint8))


def _als_args(device, fp8, k=K, degrees=DEGREES):
    indptr, indices, values = _csr(device, degrees)
    o32, obf, o8 = _outs(device, len(degrees), k)
    return dict(indptr=indptr, indices=indices, values=values,
                factors=_factors(device, fp8, k), out_f32=o32, out_bf16=obf,
                out_fp8=o8,
                row_order=torch.arange(len(degrees) - 1, -1, -1,
                                       dtype=torch.int32, device=device))


def _solve_args(device, rows=NROWS, k=K):
    g = torch.Generator().manual_seed(3)
    M = torch.randn(rows, k, k, generator=g) * 0.3
    A = (M @ M.transpose(1, 2) + 1.5 * torch.eye(k)).contiguous()
    x, xbf, x8 = _outs(device, rows, k)
    return dict(A=A.to(device), b=torch.randn(rows, k, generator=g).to(device),
                x=x, x_bf16=xbf, x_fp8=x8)


def _empty(device):
    return torch.empty(0, device=device)


def _pick(args, *names):
    return {n: args[n] for n in names}


_CSR = ("indptr", "indices", "values", "factors")


# Each entry: binding name -> (argument builder, call taking the argument
# dict and a stream, names of the tensors the binding may write).  A
# builder's dict holds exactly the tensors its call passes.
def _fused_args(fp8):
    def build(device):
        a = _als_args(device, fp8)
        # the block kernel writes the image of the gather dtype only
        a["out_bf16" if fp8 else "out_fp8"] = _empty(device)
        return a
    return build


def _call_fused(a, st):
    hip.als_solve_fused(a["indptr"], a["indices"], a["values"], a["factors"],
                        a["out_f32"], a["out_bf16"], a["out_fp8"],
                        a["row_order"], 0.3, st)


def _call_wavefused(fn):
    def call(a, st):
        fn(a["indptr"], a["indices"], a["values"], a["factors"], a["out_f32"],
           a["out_bf16"], a["out_fp8"], a["row_order"], 0.3, st)
    return call


def _gramian_args(device):
    a = _als_args(device, fp8=False)
    a = dict(_pick(a, *_CSR, "row_order"), b_out=a["out_f32"])
    a["A_out"] = torch.full((NROWS, K, K), SENTINEL, device=device)
    return a


def _call_gramian(a, st):
    hip.gramian(a["indptr"], a["indices"], a["values"], a["factors"],
                a["A_out"], a["b_out"], a["row_order"], 0.3, st)


def _call_dbg_gramian(a, st):
    hip.dbg_gramian(a["indptr"], a["indices"], a["values"], a["factors"],
                    a["A_out"], a["b_out"], a["blo"], 0.3, st)


def _dbg_gramian_args(device):
    a = _gramian_args(device)
    del a["row_order"]
    a["blo"] = torch.full((NROWS, K), SENTINEL, device=device)
    return a


def _dump_args(numel):
    def build(device):
        a = _pick(_als_args(device, fp8=False), *_CSR)
        a["out"] = torch.full((numel,), SENTINEL, device=device,
                              dtype=torch.bfloat16)
        return a
    return build


def _call_dump(fn):
    def call(a, st):
        fn(a["indptr"], a["indices"], a["values"], a["factors"], a["out"],
           st)
    return call


def _solve_args_f32_only(device):
    return _pick(_solve_args(device), "A", "b", "x")


def _call_solver(fn, lowp=True, phases=None):
    def call(a, st):
        args = [a["A"], a["b"], a["x"]]
        if lowp:
            args += [a["x_bf16"], a["x_fp8"]]
        if phases is not None:
            args.append(a.get("phases", phases))
        fn(*args, st)
    return call


def _probe_args(dt, shape_a, shape_b):
    def build(device):
        return dict(A=torch.zeros(shape_a, dtype=dt).to(device),
                    B=torch.zeros(shape_b, dtype=dt).to(device),
                    D=torch.full((16, 16), SENTINEL, device=device))
    return build


def _call_probe(fn):
    def call(a, st):
        fn(a["A"], a["B"], a["D"], st)
    return call


_ALS_OUTS = ("out_f32", "out_bf16", "out_fp8")
_SOLVE_OUTS = ("x", "x_bf16", "x_fp8")
BINDINGS = {
    "als_solve_fused": (_fused_args(False), _call_fused, _ALS_OUTS),
    "als_solve_fused[e4m3]": (_fused_args(True), _call_fused, _ALS_OUTS),
    "als_solve_wavefused": (lambda d: _als_args(d, False),
                            _call_wavefused(hip.als_solve_wavefused),
                            _ALS_OUTS),
    "als_solve_wavefused_db": (lambda d: _als_args(d, True),
                               _call_wavefused(hip.als_solve_wavefused_db),
                               _ALS_OUTS),
    "gramian": (_gramian_args, _call_gramian, ("A_out", "b_out")),
    "dbg_gramian": (_dbg_gramian_args, _call_dbg_gramian,
                    ("A_out", "b_out", "blo")),
    "dbg_stage_dump": (_dump_args((K + 16) * 32),
                       _call_dump(hip.dbg_stage_dump), ("out",)),
    "dbg_frag_dump": (_dump_args(4 * (K // 16 + 1) * 64 * 8),
                      _call_dump(hip.dbg_frag_dump), ("out",)),
    "cholesky_solve": (_solve_args_f32_only,
                       _call_solver(hip.cholesky_solve, lowp=False), ("x",)),
    "cholesky_solve_ph": (_solve_args_f32_only,
                          _call_solver(hip.cholesky_solve_ph, lowp=False,
                                       phases=3), ("x",)),
    "ldl_solve_wave": (_solve_args, _call_solver(hip.ldl_solve_wave),
                       _SOLVE_OUTS),
    "ldl_solve_wave_reg": (_solve_args,
                           _call_solver(hip.ldl_solve_wave_reg), _SOLVE_OUTS),
    "mfma_probe_f32": (_probe_args(torch.float32, (16, 4), (4, 16)),
                       _call_probe(hip.mfma_probe_f32), ("D",)),
    "mfma_probe_bf16": (_probe_args(torch.bfloat16, (32, 16), (32, 16)),
                        _call_probe(hip.mfma_probe_bf16), ("D",)),
    "mfma_probe_fp8": (_probe_args(torch.uint8, (32, 16), (32, 16)),
                       _call_probe(hip.mfma_probe_fp8), ("D",)),
}
# the first tensor each binding registers: the one a CPU call is blamed on
FIRST_ARG = {"cholesky_solve": "A", "cholesky_solve_ph": "A",
             "ldl_solve_wave": "A", "ldl_solve_wave_reg": "A",
             "mfma_probe_f32": "A", "mfma_probe_bf16": "Xt",
             "mfma_probe_fp8": "Xt"}


def _fn_name(binding):
    return binding.split("[")[0]


# ------------------------------------------------------------- CPU part

def test_broadcast_constants():
    assert hip.BROADCAST_DEFAULT == 3 and hip.BROADCAST_SHFL == 0


@pytest.mark.parametrize("binding", sorted(BINDINGS))
def test_cpu_tensors_are_rejected(binding):
    build, call, _ = BINDINGS[binding]
    with pytest.raises(RuntimeError) as ei:
        call(build("cpu"), 0)
    msg = str(ei.value)
    assert _fn_name(binding) in msg, msg
    assert FIRST_ARG.get(binding, "indptr") + " must be on the GPU" in msg, msg


def _serve_args():
    U = torch.ones(6, 16, dtype=torch.bfloat16)
    idx = torch.zeros(4, dtype=torch.int64)
    return U, U.clone(), idx, idx.clone()


def test_cpu_tensors_are_rejected_svm_and_serving():
    indptr, indices, values = _csr("cpu")
    n = NROWS
    y, w = torch.ones(n), torch.zeros(COLS)
    e = _empty("cpu")
    with pytest.raises(RuntimeError, match="sdca_pass: indptr must be on"):
        hip.sdca_pass(indptr, indices, values, y, y.clone(), e, torch.zeros(n),
                      w, 1.0, 0)
    with pytest.raises(RuntimeError, match="svm_margins: indptr must be on"):
        hip.svm_margins(indptr, indices, values, w, torch.zeros(n), 0)
    U, V, u, i = _serve_args()
    with pytest.raises(RuntimeError, match="predict_dot: U must be on"):
        hip.predict_dot(U, V, u, i, torch.zeros(4), 0)
    with pytest.raises(RuntimeError, match="sgd_update: U must be on"):
        hip.sgd_update(U, V, u, i, torch.ones(4), torch.zeros(4), 0.1, 0.1,
                       0.1, 0)


def test_cpu_wrong_dtypes_raise():
    a = _solve_args("cpu")
    a["b"] = a["b"].double()
    for name in ("cholesky_solve", "ldl_solve_wave", "ldl_solve_wave_reg"):
        with pytest.raises(RuntimeError, match="b must be"):
            BINDINGS[name][1](a, 0)
    for name in ("als_solve_fused", "als_solve_wavefused", "gramian"):
        build, call, _ = BINDINGS[name]
        a = build("cpu")
        a["indices"] = a["indices"].long()
        with pytest.raises(RuntimeError, match="indices must be"):
            call(a, 0)


@pytest.mark.parametrize("binding", ["als_solve_fused", "als_solve_fused[e4m3]",
                                     "als_solve_wavefused",
                                     "als_solve_wavefused_db"])
def test_cpu_too_few_output_rows(binding):
    """Shape checks read metadata only and run before the device check."""
    build, call, _ = BINDINGS[binding]
    a = build("cpu")
    a["out_f32"] = a["out_f32"][:NROWS - 1]
    with pytest.raises(RuntimeError, match="out_f32 must be"):
        call(a, 0)
    image = "out_bf16" if binding == "als_solve_fused" else "out_fp8"
    a = build("cpu")
    a[image] = a[image][:NROWS - 1]              # image smaller than out_f32
    with pytest.raises(RuntimeError, match=image + " must be empty or"):
        call(a, 0)


@pytest.mark.parametrize("binding", ["cholesky_solve", "cholesky_solve_ph",
                                     "ldl_solve_wave", "ldl_solve_wave_reg"])
def test_cpu_solver_shapes(binding):
    build, call, outs = BINDINGS[binding]
    for arg in ("b", "x"):
        a = build("cpu")
        a[arg] = a[arg][:NROWS - 1]
        with pytest.raises(RuntimeError, match=arg + " must be"):
            call(a, 0)
    a = build("cpu")
    a["A"] = a["A"][:, :, :K - 1].contiguous()          # not square
    with pytest.raises(RuntimeError, match=r"A must be \[n\]\[k\]\[k\]"):
        call(a, 0)
    a = _solve_args("cpu", k=24)                          # k % 16 != 0
    with pytest.raises(RuntimeError, match="multiple of 16"):
        call(a, 0)
    if "x_bf16" in outs:
        a = build("cpu")
        a["x_bf16"] = a["x_bf16"][:NROWS - 1]
        with pytest.raises(RuntimeError, match="x_bf16 must be empty or"):
            call(a, 0)


def test_cpu_misc_shapes():
    a = _solve_args("cpu")
    a["phases"] = 7
    with pytest.raises(RuntimeError, match="phases must be in 0..3"):
        BINDINGS["cholesky_solve_ph"][1](a, 0)
    a = _gramian_args("cpu")
    a["A_out"] = a["A_out"][:NROWS - 1]
    with pytest.raises(RuntimeError, match="A_out must be"):
        _call_gramian(a, 0)
    a = _fused_args(False)("cpu")
    a["row_order"] = a["row_order"][:NROWS - 1]
    with pytest.raises(RuntimeError, match="row_order must be empty or"):
        _call_fused(a, 0)
    a = _fused_args(False)("cpu")
    a["factors"] = a["factors"][:, :K - 4].contiguous()
    with pytest.raises(RuntimeError, match="multiple of 16"):
        _call_fused(a, 0)
    for name in ("dbg_stage_dump", "dbg_frag_dump"):
        build, call, _ = BINDINGS[name]
        a = build("cpu")
        a["out"] = a["out"][:-1]
        with pytest.raises(RuntimeError, match="out must have at least"):
            call(a, 0)
    for name in ("mfma_probe_f32", "mfma_probe_bf16", "mfma_probe_fp8"):
        build, call, _ = BINDINGS[name]
        a = build("cpu")
        a["D"] = torch.zeros(16, 15)
        with pytest.raises(RuntimeError, match="must have 256 elements"):
            call(a, 0)


# ------------------------------------------------------------- GPU part
# Every bad argument is at least as large in bytes as the good one, so a
# missed check could not write (or read) out of bounds.

def _wider(t):
    """Same shape, wrong dtype of the same or a larger element size."""
    if t.dtype == torch.float32:
        return t.double()
    if t.dtype == torch.int32:
        return t.long()
    if t.dtype == torch.int64:
        return t.double()
    return t.float()                                     # bf16, uint8


def _strided(t):
    """Non-contiguous view of a buffer twice the size, same shape, values."""
    if t.dim() == 1:
        return torch.stack([t, t], dim=1)[:, 0]
    return torch.cat([t, t], dim=-1)[..., : t.shape[-1]]


# sized by numel alone (flat buffers, optional images): an extra leading
# dimension changes nothing for them and is accepted
_NUMEL_SIZED = {"out_bf16", "out_fp8", "x_bf16", "x_fp8", "out", "A:probe",
                "B:probe", "D:probe"}


def _mutations(binding, args):
    probe = binding.startswith("mfma_probe")
    for name, t in args.items():
        if t.numel() == 0:
            continue                                     # an absent optional
        yield name + ":dtype", {name: _wider(t)}
        yield name + ":strided", {name: _strided(t)}
        if (name + ":probe" if probe else name) not in _NUMEL_SIZED:
            yield name + ":leading-dim", {name: t.unsqueeze(0)}
    if "row_order" in args:
        ro = args["row_order"]
        yield "row_order:too-long", {"row_order": torch.cat([ro, ro[:1]])}
    if binding == "cholesky_solve_ph":
        yield "phases=7", {"phases": 7}
    if binding.startswith("als_solve_fused"):
        # the image of the OTHER dtype, non-empty and full-sized
        _, obf, o8 = _outs(args["out_f32"].device)
        fp8 = args["factors"].dtype == torch.uint8
        yield "mismatched-image", ({"out_bf16": obf} if fp8
                                   else {"out_fp8": o8})
    if probe:
        yield "A:numel", {"A": torch.cat([args["A"], args["A"]])}


@pytest.mark.parametrize("binding", sorted(BINDINGS))
def test_cpu_bad_arguments_fail_a_metadata_check(binding):
    """Every bad argument of the GPU part is caught by a dtype, layout or
    shape check, which come before (and so are not) the device check."""
    build, call, _ = BINDINGS[binding]
    good = build("cpu")
    for what, change in _mutations(binding, good):
        with pytest.raises(RuntimeError) as ei:
            call(dict(good, **change), 0)
        assert "must be on the GPU" not in str(ei.value), (what, ei.value)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("binding", sorted(BINDINGS))
def test_gpu_bad_arguments_raise_and_write_nothing(gpu, binding):
    build, call, outs = BINDINGS[binding]
    good = build(gpu)
    cases = list(_mutations(binding, good))
    assert len(cases) >= 3
    for what, change in cases:
        a = dict(good, **change)
        before = {n: a[n].clone() for n in outs}
        with pytest.raises(RuntimeError):
            call(a, _stream())
        torch.cuda.synchronize()
        for n in outs:
            assert torch.equal(a[n], before[n]), (binding, what, n)
            assert torch.equal(good[n], before[n]) or n in change, \
                (binding, what, n)


def _bits(outs):
    return [o.view(torch.int16) if o.dtype == torch.bfloat16 else
            o.view(torch.int32) if o.dtype == torch.float32 else o
            for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("binding", ["als_solve_wavefused",
                                     "als_solve_wavefused_db",
                                     "ldl_solve_wave_reg"])
def test_gpu_variantless_call_runs_the_default(gpu, binding):
    build, _, outs = BINDINGS[binding]
    fn = getattr(hip, binding)
    got = []
    for extra in ((), (hip.BROADCAST_DEFAULT,)):
        a = build(gpu)
        if binding == "ldl_solve_wave_reg":
            fn(a["A"], a["b"], a["x"], a["x_bf16"], a["x_fp8"], _stream(),
               *extra)
        else:
            fn(a["indptr"], a["indices"], a["values"], a["factors"],
               a["out_f32"], a["out_bf16"], a["out_fp8"], a["row_order"], 0.3,
               _stream(), *extra)
        torch.cuda.synchronize()
        got.append(_bits([a[n] for n in outs]))
    for x, y in zip(*got):
        assert torch.equal(x, y)
    assert torch.isfinite(got[0][0].view(torch.float32)).all()
    assert (got[0][0].view(torch.float32) != SENTINEL).all()


@pytest.mark.gpu
def test_gpu_wavefused_accepts_a_taller_output(gpu):
    """The outputs may have more rows than the launch covers (the chunked
    path scatters into full-side buffers with this kernel): same rows as an
    exact-size call, the extra rows untouched."""
    k, degrees = 64, [0, 1, 33, 65]
    call = _call_wavefused(hip.als_solve_wavefused)
    exact = _als_args(gpu, True, k=k, degrees=degrees)
    call(exact, _stream())
    tall = _als_args(gpu, True, k=k, degrees=degrees)
    tall["out_f32"], tall["out_bf16"], tall["out_fp8"] = _outs(
        gpu, len(degrees) + 2, k)
    call(tall, _stream())
    torch.cuda.synchronize()
    n = len(degrees)
    for name in _ALS_OUTS:
        assert torch.equal(_bits([tall[name][:n]])[0],
                           _bits([exact[name]])[0]), name
    assert (tall["out_f32"][n:] == SENTINEL).all()
    assert (tall["out_bf16"][n:] == SENTINEL).all()
    assert (tall["out_fp8"][n:] == 0x7F).all()
    assert torch.isfinite(exact["out_f32"]).all()
    assert exact["out_f32"][0].abs().sum() == 0      # the degree-0 entity
    assert (exact["out_f32"][1:] != SENTINEL).all()
