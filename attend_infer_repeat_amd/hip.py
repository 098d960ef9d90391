"""Tensor-level entry points over the C ABI (include/air_hip.h): argument checking, output allocation and stream
plumbing only -- all arithmetic happens in libair_hip.so.  No autograd here (see functional.py) and no fallback:
CPU tensors are rejected.

torch is used for device memory and the current HIP stream, nothing else.
"""
import ctypes

import torch

from . import _lib

ACT_NONE, ACT_ELU = 0, 1
EPI_NONE, EPI_BIAS, EPI_BIAS_ELU, EPI_MUL_DELU, EPI_ADD_AUX, EPI_ADD_AUX_ELU = 0, 1, 2, 3, 4, 5

_WS = {}
_WS_BYTES = 64 << 20


def lib():
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name, dims=None):
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.AirHipError(f"{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.AirHipError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.AirHipError(f"{name}: expected a contiguous tensor")
    if dims is not None and t.dim() != dims:
        raise _lib.AirHipError(f"{name}: expected {dims} dims, got shape {tuple(t.shape)}")
    return t


def workspace(device=None):
    """Split-K workspace shared by every GEMM on a device (allocated once, outside any graph capture)."""
    dev = torch.device(device if device is not None else torch.cuda.current_device())
    if dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _WS:
        _WS[key] = torch.empty(_WS_BYTES // 4, dtype=torch.float32, device=torch.device("cuda", key))
    return _WS[key]


def _ws_args(t):
    ws = workspace(t.device)
    return _p(ws), ctypes.c_size_t(ws.numel() * 4)


# ---- spatial transformer ----------------------------------------------------------------------------------------
def st_read_fwd(img, where, crop_size, n_img=None):
    img = _f32(img, "img", 3); where = _f32(where, "where", 2)
    n_images, H, W = img.shape
    n = where.shape[0]
    h, w = int(crop_size[0]), int(crop_size[1])
    out = torch.empty((n, h, w), dtype=torch.float32, device=img.device)
    _lib.check(lib().air_st_read_fwd(_p(img), _p(where), _p(out), n, n_images if n_img is None else n_img, H, W, h,
                                     w, _stream()), "air_st_read_fwd")
    return out


def st_read_bwd(img, where, dglimpse, want_dimg=False):
    img = _f32(img, "img", 3); where = _f32(where, "where", 2); dglimpse = _f32(dglimpse, "dglimpse", 3)
    n_images, H, W = img.shape
    n, h, w = dglimpse.shape
    dwhere = torch.empty((n, 4), dtype=torch.float32, device=img.device)
    dimg = torch.empty_like(img) if want_dimg else None
    _lib.check(lib().air_st_read_bwd(_p(img), _p(where), _p(dglimpse), _p(dwhere), _p(dimg), n, n_images, H, W, h, w,
                                     _stream()), "air_st_read_bwd")
    return dwhere, dimg


def st_write_fwd(glimpse, where, img_size, presence=None, canvas_in=None):
    glimpse = _f32(glimpse, "glimpse", 3); where = _f32(where, "where", 2)
    presence = _f32(presence, "presence"); canvas_in = _f32(canvas_in, "canvas_in")
    n, h, w = glimpse.shape
    H, W = int(img_size[0]), int(img_size[1])
    out = torch.empty((n, H, W), dtype=torch.float32, device=glimpse.device)
    _lib.check(lib().air_st_write_fwd(_p(glimpse), _p(where), _p(presence), _p(canvas_in), _p(out), n, H, W, h, w,
                                      _stream()), "air_st_write_fwd")
    return out


def st_write_bwd(glimpse, where, dcanvas, presence=None, want_dpresence=False):
    glimpse = _f32(glimpse, "glimpse", 3); where = _f32(where, "where", 2); dcanvas = _f32(dcanvas, "dcanvas", 3)
    presence = _f32(presence, "presence")
    n, h, w = glimpse.shape
    H, W = dcanvas.shape[1:]
    dg = torch.empty_like(glimpse)
    dwhere = torch.empty((n, 4), dtype=torch.float32, device=glimpse.device)
    dpres = torch.empty((n,), dtype=torch.float32, device=glimpse.device) if want_dpresence else None
    _lib.check(lib().air_st_write_bwd(_p(glimpse), _p(where), _p(presence), _p(dcanvas), _p(dg), _p(dwhere),
                                      _p(dpres), n, H, W, h, w, _stream()), "air_st_write_bwd")
    return dg, dwhere, dpres


def canvas_unroll_fwd(glimpse, where, presence, img_size, obs=None, mult=1.0, std=1.0, keep_steps=True):
    """glimpse[T,B,h,w], where[T,B,4], presence[T,B] -> (canvas_steps[T,B,H,W] | None, final[B,H,W], rec[B] | None)"""
    glimpse = _f32(glimpse, "glimpse", 4); where = _f32(where, "where", 3); presence = _f32(presence, "presence")
    obs = _f32(obs, "obs")
    T, B, h, w = glimpse.shape
    H, W = int(img_size[0]), int(img_size[1])
    dev = glimpse.device
    steps = torch.empty((T, B, H, W), dtype=torch.float32, device=dev) if keep_steps else None
    final = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    rec = torch.empty((B,), dtype=torch.float32, device=dev) if obs is not None else None
    _lib.check(lib().air_canvas_unroll_fwd(_p(glimpse), _p(where), _p(presence), _p(obs), _p(steps), _p(final),
                                           _p(rec), T, B, H, W, h, w, float(mult), float(std), _stream()),
               "air_canvas_unroll_fwd")
    return steps, final, rec


def canvas_unroll_bwd(glimpse, where, presence, obs, final_canvas, mult, std, loss_scale):
    """final_canvas=None: the recompute form (every (t, b) unit re-forms the canvas on its own footprint from the T glimpses of
    its image, bit-identically to the forward) -- the backward then does not depend on the forward launch."""
    glimpse = _f32(glimpse, "glimpse", 4); where = _f32(where, "where", 3); presence = _f32(presence, "presence")
    obs = _f32(obs, "obs", 3)
    final_canvas = _f32(final_canvas, "final_canvas", 3) if final_canvas is not None else None
    T, B, h, w = glimpse.shape
    H, W = obs.shape[1:]
    dg = torch.empty_like(glimpse)
    dwhere = torch.empty((T, B, 4), dtype=torch.float32, device=glimpse.device)
    _lib.check(lib().air_canvas_unroll_bwd(_p(glimpse), _p(where), _p(presence), _p(obs), _p(final_canvas), _p(dg),
                                           _p(dwhere), T, B, H, W, h, w, float(mult), float(std), float(loss_scale),
                                           _stream()), "air_canvas_unroll_bwd")
    return dg, dwhere


# ---- which kernel a read / canvas launch runs (host-only queries: no launch, no device memory) ---------------------------------
def _addr(x):
    """an operand of a form query: a tensor, an integer ADDRESS (only its alignment and NULL-ness matter) or None"""
    if x is None:
        return None
    return ctypes.c_void_p(x.data_ptr() if torch.is_tensor(x) else int(x))


def _warp_form(name, *args):
    f = _lib.AirWarpForm()
    st = getattr(lib(), name)(*args, ctypes.byref(f))
    d = f.as_dict()
    d["kernel"] = _lib.WARP_KERNELS[d["kernel"]]
    return st, d


def st_read_form(img, where, glimpse, n, n_img, H, W, h, w):
    """air_st_read_form: which kernel air_st_read_fwd runs -> (status, dict over the fields of AirWarpForm)"""
    return _warp_form("air_st_read_form", _addr(img), _addr(where), _addr(glimpse), n, n_img, H, W, h, w)


def st_read_bwd_form(img, where, dglimpse, dwhere, dimg, n, n_img, H, W, h, w):
    """air_st_read_bwd_form -> (status, form)"""
    return _warp_form("air_st_read_bwd_form", _addr(img), _addr(where), _addr(dglimpse), _addr(dwhere), _addr(dimg), n, n_img, H, W, h, w)


def canvas_fwd_form(glimpse, where, obs, canvas_steps, final_canvas, rec_parts, n_bands, T, B, H, W, h, w):
    """air_canvas_fwd_form -> (status, form): air_st_write_fwd (T = 1, n_bands = 1), air_canvas_unroll_fwd (n_bands = 0) and
    air_canvas_unroll_fwd_banded (n_bands > 0)"""
    return _warp_form("air_canvas_fwd_form", _addr(glimpse), _addr(where), _addr(obs), _addr(canvas_steps), _addr(final_canvas),
                      _addr(rec_parts), n_bands, T, B, H, W, h, w)


def canvas_bwd_form(glimpse, where, dcanvas, final_canvas, obs, dglimpse, dwhere, T, B, H, W, h, w):
    """air_canvas_bwd_form -> (status, form): air_st_write_bwd (dcanvas given, T = 1) and air_canvas_unroll_bwd / _dpresence / _nvil"""
    return _warp_form("air_canvas_bwd_form", _addr(glimpse), _addr(where), _addr(dcanvas), _addr(final_canvas), _addr(obs),
                      _addr(dglimpse), _addr(dwhere), T, B, H, W, h, w)


def canvas_fwd_bwd_form(glimpse, where, obs, canvas_steps, final_canvas, rec_parts, n_bands, dglimpse, dwhere, n_split, T, B, H, W, h, w):
    """air_canvas_fwd_bwd_form -> (status, form) of air_canvas_unroll_fwd_bwd"""
    return _warp_form("air_canvas_fwd_bwd_form", _addr(glimpse), _addr(where), _addr(obs), _addr(canvas_steps), _addr(final_canvas),
                      _addr(rec_parts), n_bands, _addr(dglimpse), _addr(dwhere), n_split, T, B, H, W, h, w)


# ---- dense ---------------------------------------------------------------------------------------------------------
def gemm(A, B, ta=False, tb=False, bias=None, epilogue=EPI_NONE, aux=None, beta=0.0, out=None, colsum=False,
         use_workspace=True, precision=0, ws_bytes=None):
    """C = epi(op(A).op(B) + beta*C).  A, B: 2-D tensors whose last stride is 1 (row views with a leading dimension
    are fine).  Returns C (and the column sums of op(B) when colsum is True or a tensor to write them into).  precision=1:
    air_gemm_bf16 (operands rounded to bf16 in registers).  out: a caller-owned [M, N] view (any leading dimension);
    ws_bytes: offer only that much of the workspace (caps the K split)."""
    for t, nm in ((A, "A"), (B, "B")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
            raise _lib.AirHipError(f"gemm: {nm} must be a 2-D float32 CUDA tensor with unit inner stride")
    if precision not in (0, 1):
        raise _lib.AirHipError(f"gemm: precision {precision} is neither 0 (fp32) nor 1 (bf16)")
    M = A.shape[1] if ta else A.shape[0]
    K = A.shape[0] if ta else A.shape[1]
    Kb = B.shape[1] if tb else B.shape[0]
    N = B.shape[0] if tb else B.shape[1]
    if K != Kb:
        raise _lib.AirHipError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    lda = A.stride(0) if A.shape[0] > 1 else A.shape[1]
    ldb = B.stride(0) if B.shape[0] > 1 else B.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    ldc = out.stride(0) if out.shape[0] > 1 else out.shape[1]
    ldaux = 0
    if aux is not None:
        ldaux = aux.stride(0) if aux.shape[0] > 1 else aux.shape[1]
    cs = colsum if torch.is_tensor(colsum) else (torch.empty((N,), dtype=torch.float32, device=A.device) if colsum else None)
    wsp, wsb = _ws_args(A) if use_workspace else (None, ctypes.c_size_t(0))
    if use_workspace and ws_bytes is not None:
        wsb = ctypes.c_size_t(min(int(ws_bytes), wsb.value))
    name = "air_gemm_bf16" if precision else "air_gemm"
    _lib.check(getattr(lib(), name)(int(ta), int(tb), M, N, K, _p(A), lda, _p(B), ldb, _p(out), ldc, _p(bias),
                                    int(epilogue), _p(aux), ldaux, float(beta), _p(cs), wsp, wsb, _stream()), name)
    return (out, cs) if cs is not None else out


def gemm_form(M, N, K, colsum=False, ws_bytes=_WS_BYTES):
    """air_gemm_form: which kernel air_gemm / air_gemm_bf16 run on [M, N, K] -> dict over the fields of AirGemmForm (no launch)"""
    f = _lib.AirGemmForm()
    _lib.check(lib().air_gemm_form(M, N, K, int(bool(colsum)), ctypes.c_size_t(ws_bytes), ctypes.byref(f)), "air_gemm_form")
    return f.as_dict()


def gemm_grouped_form(problems, precision=0):
    """air_gemm_grouped_form: which kernel air_gemm_grouped runs the problems on -> (status, dict over the fields of AirGemmForm)"""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped_form")
    f = _lib.AirGemmForm()
    st = int(lib().air_gemm_grouped_form(arr, len(outs), ctypes.byref(f)))
    return st, f.as_dict()


def _gemm_descs(problems, precision, name):
    """problem dicts (see gemm_grouped) -> (AirGemmDesc array, [(C, colsum|None)], the tensors the array points into).  `colsum` may be
    True (allocated here) or a tensor to write into (a slice of a flat gradient buffer)."""
    descs, outs, keep = [], [], []
    for pr in problems:
        A, B = pr["A"], pr["B"]
        ta, tb = bool(pr.get("ta", False)), bool(pr.get("tb", False))
        M = A.shape[1] if ta else A.shape[0]
        K = A.shape[0] if ta else A.shape[1]
        N = B.shape[0] if tb else B.shape[1]
        out = pr.get("out")
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        aux, bias = pr.get("aux"), pr.get("bias")
        cs = pr.get("colsum")
        if not torch.is_tensor(cs):
            cs = torch.empty((N,), dtype=torch.float32, device=A.device) if cs else None
        ld = lambda t: t.stride(0) if t.shape[0] > 1 else t.shape[1]
        d = _lib.AirGemmDesc(int(ta), int(tb), M, N, K, A.data_ptr(), ld(A), B.data_ptr(), ld(B), out.data_ptr(), ld(out),
                             bias.data_ptr() if bias is not None else None, int(pr.get("epilogue", EPI_NONE)),
                             aux.data_ptr() if aux is not None else None, ld(aux) if aux is not None else 0,
                             float(pr.get("beta", 0.0)), cs.data_ptr() if cs is not None else None, int(precision),
                             pr["A2"].data_ptr() if pr.get("A2") is not None else None,
                             pr["a_bias"].data_ptr() if pr.get("a_bias") is not None else None, int(bool(pr.get("a_elu", False))),
                             pr["a_out"].data_ptr() if pr.get("a_out") is not None else None)
        for fld in ("A16", "B16", "C16"):
            t = pr.get(fld)
            if t is not None:
                if t.dtype != torch.bfloat16 or not t.is_cuda:
                    raise _lib.AirHipError(f"{name}: {fld} must be a bfloat16 CUDA tensor")
                setattr(d, fld, t.data_ptr())
        descs.append(d); outs.append((out, cs)); keep.append((A, B, aux, bias, pr.get("A16"), pr.get("B16"), pr.get("C16")))
    return (_lib.AirGemmDesc * len(descs))(*descs), outs, keep


def gemm_grouped(problems, precision=0):
    """Several independent GEMMs in one launch (air_gemm_grouped).  problems: dicts with A, B and optional ta, tb, bias,
    epilogue, aux, beta, out, colsum (bool); a single problem may carry the K-split consumer prologue A2, a_bias, a_elu, a_out
    (a = act(A + A2 + a_bias), see AirGemmDesc).  bf16 data path (precision=1): A16 / B16 = bf16 mirrors of A / B (same shape
    and strides in elements), C16 = bf16 tensor that receives bf16(C).  Returns [(C, colsum|None)]."""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped")
    _lib.check(lib().air_gemm_grouped(arr, len(outs), _stream()), "air_gemm_grouped")
    return outs


def linear_fwd(x, w, b, act, out=None):
    """y = act(x . w + b); out: a caller-owned contiguous [M, N] tensor for y"""
    x = _f32(x, "x", 2); w = _f32(w, "w", 2); b = _f32(b, "b")
    M, K = x.shape
    N = w.shape[1]
    if w.shape[0] != K:
        raise _lib.AirHipError(f"linear: x is [{M},{K}] but w is {tuple(w.shape)}")
    y = torch.empty((M, N), dtype=torch.float32, device=x.device) if out is None else _f32(out, "out", 2)
    if tuple(y.shape) != (M, N):
        raise _lib.AirHipError(f"linear: out is {tuple(y.shape)}, expected {(M, N)}")
    wsp, wsb = _ws_args(x)
    _lib.check(lib().air_linear_fwd(_p(x), _p(w), _p(b), _p(y), M, K, N, int(act), wsp, wsb, _stream()),
               "air_linear_fwd")
    return y


def linear_bwd(x, w, y, dy, act, want_dx=True, want_db=True, out=None):
    """-> dx, dw, db; out: caller-owned contiguous (dx[M, K] | None, dw[K, N], db[N] | None) to write into"""
    x = _f32(x, "x", 2); w = _f32(w, "w", 2); dy = _f32(dy, "dy", 2); y = _f32(y, "y")
    M, K = x.shape
    N = w.shape[1]
    if out is not None:
        dx, dw, db = (_f32(t, "out") for t in out)
        if (dx is not None and dx.shape != x.shape) or dw.shape != w.shape or (db is not None and tuple(db.shape) != (N,)):
            raise _lib.AirHipError("linear_bwd: out does not match (dx[M, K], dw[K, N], db[N])")
    else:
        dx = torch.empty_like(x) if want_dx else None
        dw = torch.empty_like(w)
        db = torch.empty((N,), dtype=torch.float32, device=x.device) if want_db else None
    gbuf = torch.empty_like(dy) if act != ACT_NONE else None
    wsp, wsb = _ws_args(x)
    _lib.check(lib().air_linear_bwd(_p(x), _p(w), _p(y), _p(dy), _p(dx), _p(dw), _p(db), _p(gbuf), M, K, N, int(act),
                                    wsp, wsb, _stream()), "air_linear_bwd")
    return dx, dw, db


def _lstm_out(out, shapes, device):
    """the caller's output buffers (a tuple, so that a test can prime and pad what a launch writes), or fresh ones of `shapes`
    (None: an output the launch is not asked for)"""
    if out is None:
        return tuple(torch.empty(s, dtype=torch.float32, device=device) if s is not None else None for s in shapes)
    if len(out) != len(shapes):
        raise _lib.AirHipError(f"expected {len(shapes)} output buffers, got {len(out)}")
    for o, s in zip(out, shapes):
        if (o is None) != (s is None) or (o is not None and tuple(_f32(o, "out").shape) != tuple(s)):
            raise _lib.AirHipError("an output buffer does not match the shape the launch writes")
    return tuple(out)


def lstm_pointwise_fwd(gates, c_prev, forget_bias=1.0, out=None, want_act=True):
    """out = (h, c, gate_act): caller-owned buffers; want_act=False: gate_act = NULL"""
    gates = _f32(gates, "gates", 2); c_prev = _f32(c_prev, "c_prev", 2)
    M, Hd = c_prev.shape
    h, c, act = _lstm_out(out, ((M, Hd), (M, Hd), (M, 4 * Hd) if want_act else None), c_prev.device)
    _lib.check(lib().air_lstm_pointwise_fwd(_p(gates), _p(c_prev), _p(h), _p(c), _p(act), M, Hd, float(forget_bias),
                                            _stream()), "air_lstm_pointwise_fwd")
    return h, c, act


def lstm_pointwise_bwd(gate_act, c_prev, c, dh, dc, dh2=None, out=None):
    """out = (dgates, dc_prev): caller-owned buffers"""
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    dh = _f32(dh, "dh"); dc = _f32(dc, "dc"); dh2 = _f32(dh2, "dh2")
    M, Hd = c_prev.shape
    dgates, dc_prev = _lstm_out(out, ((M, 4 * Hd), (M, Hd)), c_prev.device)
    _lib.check(lib().air_lstm_pointwise_bwd(_p(gate_act), _p(c_prev), _p(c), _p(dh), _p(dh2), _p(dc), _p(dgates),
                                            _p(dc_prev), M, Hd, _stream()), "air_lstm_pointwise_bwd")
    return dgates, dc_prev


def _bf16(t, name, shape=None):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise _lib.AirHipError(f"{name}: expected a contiguous bfloat16 CUDA tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.AirHipError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def lstm_pointwise_bwd_bf16(gate_act, c_prev, c, dh, dc, dgates_bf16, dh2=None, out=None):
    """air_lstm_pointwise_bwd_bf16: air_lstm_pointwise_bwd that also writes the bf16 mirror of dgates -> dgates, dc_prev"""
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    dh = _f32(dh, "dh"); dc = _f32(dc, "dc"); dh2 = _f32(dh2, "dh2")
    M, Hd = c_prev.shape
    _bf16(dgates_bf16, "dgates_bf16", (M, 4 * Hd))
    dgates, dc_prev = _lstm_out(out, ((M, 4 * Hd), (M, Hd)), c_prev.device)
    _lib.check(lib().air_lstm_pointwise_bwd_bf16(_p(gate_act), _p(c_prev), _p(c), _p(dh), _p(dh2), _p(dc), _p(dgates), _p(dgates_bf16),
                                                 _p(dc_prev), M, Hd, _stream()), "air_lstm_pointwise_bwd_bf16")
    return dgates, dc_prev


def lstm_step_fwd(h_prev, c_prev, w_h, gx, forget_bias=1.0, precision=0, out=None):
    """fused recurrent product + gate math: (h, c, gate_act) from h_prev[M,Hd], c_prev[M,Hd], w_h[Hd,4Hd], gx[M,4Hd] (w_h and gx may
    be row views of wider buffers); out = (h, c, gate_act): caller-owned buffers"""
    h_prev = _f32(h_prev, "h_prev", 2); c_prev = _f32(c_prev, "c_prev", 2)
    M, Hd = c_prev.shape
    ldgx = _mat(gx, "gx", 4 * Hd)
    if not (w_h.is_cuda and w_h.dtype == torch.float32 and w_h.dim() == 2 and w_h.stride(1) == 1):
        raise ValueError("w_h must be a row-major fp32 CUDA matrix (row stride allowed)")
    h, c, act = _lstm_out(out, ((M, Hd), (M, Hd), (M, 4 * Hd)), c_prev.device)
    _lib.check(lib().air_lstm_step_fwd(_p(h_prev), _p(c_prev), _p(w_h), w_h.stride(0), _p(gx), ldgx, _p(h), _p(c),
                                       _p(act), M, Hd, float(forget_bias), int(precision), _stream()), "air_lstm_step_fwd")
    return h, c, act


def lstm_step_fwd_bf16(h_prev, c_prev, w_h_bf16, gx, forget_bias=1.0, h_prev_bf16=None, h_bf16=None, out=None):
    """air_lstm_step_fwd_bf16: W_h from its bf16 shadow [Hd, 4Hd], h_prev from its bf16 mirror where one is given, the bf16 mirror of
    h written where one is given -> h, c, gate_act"""
    h_prev = _f32(h_prev, "h_prev", 2); c_prev = _f32(c_prev, "c_prev", 2)
    M, Hd = c_prev.shape
    ldgx = _mat(gx, "gx", 4 * Hd)
    _bf16(w_h_bf16, "w_h_bf16", (Hd, 4 * Hd)); _bf16(h_prev_bf16, "h_prev_bf16", (M, Hd)); _bf16(h_bf16, "h_bf16", (M, Hd))
    h, c, act = _lstm_out(out, ((M, Hd), (M, Hd), (M, 4 * Hd)), c_prev.device)
    _lib.check(lib().air_lstm_step_fwd_bf16(_p(h_prev), _p(h_prev_bf16), _p(c_prev), _p(w_h_bf16), 4 * Hd, _p(gx), ldgx, _p(h), _p(h_bf16),
                                            _p(c), _p(act), M, Hd, float(forget_bias), _stream()), "air_lstm_step_fwd_bf16")
    return h, c, act


def lstm_step_bwd(dgates_next, w_h, dh_a, dh_b, dc_in, gate_act, c_prev, c, dgx_in=None, want_dgx=False, precision=0, out=None):
    """fused BPTT link: dh = dgates_next . w_h^T + dh_a + dh_b, then the pointwise backward -> dgates, dc_prev[, dgx];
    out = (dgates, dc_prev, dgx | None): caller-owned buffers (dgx may be dgx_in itself: the running sum in place)"""
    dgates_next = _f32(dgates_next, "dgates_next", 2); w_h = _f32(w_h, "w_h", 2)
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    M, Hd = c_prev.shape
    dgates, dc_prev, dgx = _lstm_out(out, ((M, 4 * Hd), (M, Hd), (M, 4 * Hd) if (want_dgx if out is None else out[2] is not None) else None),
                                      c_prev.device)
    _lib.check(lib().air_lstm_step_bwd(_p(dgates_next), _p(w_h), _p(dh_a), _p(dh_b), _p(dc_in), _p(gate_act), _p(c_prev),
                                       _p(c), _p(dgx_in), _p(dgates), _p(dc_prev), _p(dgx), M, Hd, int(precision),
                                       _stream()), "air_lstm_step_bwd")
    return dgates, dc_prev, dgx


def lstm_step_bwd_bf16(dgates_next, w_h_bf16, dh_a, dh_b, dc_in, gate_act, c_prev, c, dgx_in=None, dgates_next_bf16=None, dgates_bf16=None,
                       dgx_bf16=None, out=None):
    """air_lstm_step_bwd_bf16: the link with W_h from its bf16 shadow, dgates_next from its mirror where one is given, and the mirrors
    of dgates / the running dgx written where given; out = (dgates, dc_prev, dgx | None) -> dgates, dc_prev, dgx"""
    dgates_next = _f32(dgates_next, "dgates_next", 2)
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    M, Hd = c_prev.shape
    _bf16(w_h_bf16, "w_h_bf16", (Hd, 4 * Hd))
    for t, nm in ((dgates_next_bf16, "dgates_next_bf16"), (dgates_bf16, "dgates_bf16"), (dgx_bf16, "dgx_bf16")):
        _bf16(t, nm, (M, 4 * Hd))
    dgates, dc_prev, dgx = _lstm_out(out, ((M, 4 * Hd), (M, Hd), (M, 4 * Hd) if (out is None or out[2] is not None) else None), c_prev.device)
    _lib.check(lib().air_lstm_step_bwd_bf16(_p(dgates_next), _p(dgates_next_bf16), _p(w_h_bf16), _p(dh_a), _p(dh_b), _p(dc_in), _p(gate_act),
                                            _p(c_prev), _p(c), _p(dgx_in), _p(dgates), _p(dgates_bf16), _p(dc_prev), _p(dgx), _p(dgx_bf16),
                                            M, Hd, _stream()), "air_lstm_step_bwd_bf16")
    return dgates, dc_prev, dgx


def rmsprop_slice(p, g, ms, mg, mom, lo, hi, n_model, lr_dev, lr_mult_tail=1.0, decay=0.9, momentum=0.9, eps=1e-10,
                  grad_scale=1.0):
    """AirRmspropSlice over the flat buffers: elements [lo, hi) are updated by the *_opt launch the slice is handed to."""
    for t, nm in ((p, "p"), (g, "g"), (ms, "ms"), (mg, "mg"), (mom, "mom"), (lr_dev, "lr_dev")):
        _f32(t, nm)
    return _lib.AirRmspropSlice(p.data_ptr(), g.data_ptr(), ms.data_ptr(), mg.data_ptr(), mom.data_ptr(), int(lo), int(hi),
                                int(n_model), lr_dev.data_ptr(), float(lr_mult_tail), float(decay), float(momentum), float(eps),
                                float(grad_scale))


def lstm_pointwise_bwd_opt(gate_act, c_prev, c, dh, dc, opt):
    """air_lstm_pointwise_bwd with an optimiser slice (rmsprop_slice(...)) riding as extra workgroups of the launch"""
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    dh = _f32(dh, "dh"); dc = _f32(dc, "dc")
    M, Hd = c_prev.shape
    dgates = torch.empty_like(gate_act); dc_prev = torch.empty_like(c_prev)
    _lib.check(lib().air_lstm_pointwise_bwd_opt(_p(gate_act), _p(c_prev), _p(c), _p(dh), None, _p(dc), _p(dgates),
                                                _p(dc_prev), M, Hd, ctypes.byref(opt) if opt is not None else None, _stream()),
               "air_lstm_pointwise_bwd_opt")
    return dgates, dc_prev


def lstm_step_bwd_opt(dgates_next, w_h, dh_a, dh_b, dc_in, gate_act, c_prev, c, opt, precision=0, out=None):
    """air_lstm_step_bwd with an optimiser slice riding along; out = (dgates, dc_prev): caller-owned buffers"""
    dgates_next = _f32(dgates_next, "dgates_next", 2); w_h = _f32(w_h, "w_h", 2)
    gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    M, Hd = c_prev.shape
    dgates, dc_prev = _lstm_out(out, ((M, 4 * Hd), (M, Hd)), c_prev.device)
    _lib.check(lib().air_lstm_step_bwd_opt(_p(dgates_next), _p(w_h), _p(dh_a), _p(dh_b), _p(dc_in), _p(gate_act), _p(c_prev),
                                           _p(c), None, _p(dgates), _p(dc_prev), None, M, Hd, int(precision),
                                           ctypes.byref(opt) if opt is not None else None, _stream()), "air_lstm_step_bwd_opt")
    return dgates, dc_prev


def lstm_step_bwd_entry(gate_act1, c_prev1, c1, dh_a1, dh_b1, w_h, dh_a, dh_b, gate_act, c_prev, c, opt=None, want_dgx=True, out=None):
    """air_lstm_step_bwd_entry: pointwise backward of the last step + the first BPTT link in one launch.
    out = (dgates1, dc_prev1, dgates, dc_prev, dgx | None): caller-owned buffers.  Returns (dgates1, dc_prev1, dgates, dc_prev, dgx)"""
    gate_act1 = _f32(gate_act1, "gate_act1", 2); c_prev1 = _f32(c_prev1, "c_prev1", 2); c1 = _f32(c1, "c1", 2)
    w_h = _f32(w_h, "w_h", 2); gate_act = _f32(gate_act, "gate_act", 2); c_prev = _f32(c_prev, "c_prev", 2); c = _f32(c, "c", 2)
    M, Hd = c_prev.shape
    dgates1, dc_prev1, dgates, dc_prev, dgx = _lstm_out(out, ((M, 4 * Hd), (M, Hd), (M, 4 * Hd), (M, Hd),
                                                              (M, 4 * Hd) if (want_dgx if out is None else out[4] is not None) else None),
                                                        c_prev.device)
    _lib.check(lib().air_lstm_step_bwd_entry(_p(gate_act1), _p(c_prev1), _p(c1), _p(dh_a1), _p(dh_b1), _p(dgates1), _p(dc_prev1),
                                             _p(w_h), _p(dh_a), _p(dh_b), _p(gate_act), _p(c_prev), _p(c), _p(dgates), _p(dc_prev),
                                             _p(dgx), M, Hd, ctypes.byref(opt) if opt is not None else None, _stream()),
               "air_lstm_step_bwd_entry")
    return dgates1, dc_prev1, dgates, dc_prev, dgx


# ---- stochastic nodes ----------------------------------------------------------------------------------------------
def gauss_sample_fwd(pre, eps, raw_offset, loc_mode, prior4, want_kl=True, guard_eps=0.0):
    """pre[M, >=2D] (row stride allowed), eps[M,D] or None -> loc, scale, sample|None, kl_row|None
    guard_eps > 0: the stability switch of include/air_hip.h (scale floor, |where scale| >= guard_eps); 0 = the reference's arithmetic"""
    if not (pre.is_cuda and pre.dtype == torch.float32 and pre.dim() == 2 and pre.stride(1) == 1):
        raise _lib.AirHipError("gauss_sample: pre must be a 2-D float32 CUDA tensor with unit inner stride")
    eps = _f32(eps, "eps")
    M = pre.shape[0]
    D = pre.shape[1] // 2
    ld = pre.stride(0) if M > 1 else pre.shape[1]
    dev = pre.device
    loc = torch.empty((M, D), dtype=torch.float32, device=dev); scale = torch.empty_like(loc)
    sample = torch.empty_like(loc) if eps is not None else None
    kl = torch.empty((M,), dtype=torch.float32, device=dev) if want_kl else None
    a, b, c, d = (float(v) for v in prior4)
    _lib.check(lib().air_gauss_sample_fwd(_p(pre), ld, _p(eps), float(raw_offset), int(loc_mode), a, b, c, d, _p(loc),
                                          _p(scale), _p(sample), _p(kl), M, D, float(guard_eps), _stream()), "air_gauss_sample_fwd")
    return loc, scale, sample, kl


def gauss_sample_bwd(pre, eps, raw_offset, loc_mode, prior4, loc, scale, dsample, dkl_row, guard_eps=0.0):
    M, D = loc.shape
    ld = pre.stride(0) if M > 1 else pre.shape[1]
    dpre = torch.empty((M, 2 * D), dtype=torch.float32, device=pre.device)
    a, b, c, d = (float(v) for v in prior4)
    _lib.check(lib().air_gauss_sample_bwd(_p(pre), ld, _p(eps), float(raw_offset), int(loc_mode), a, b, c, d, _p(loc),
                                          _p(scale), _p(_f32(dsample, "dsample")), None, _p(_f32(dkl_row, "dkl_row")),
                                          1.0, _p(dpre), 2 * D, M, D, float(guard_eps), None, 0, None, _stream()), "air_gauss_sample_bwd")
    return dpre


def normal_kl_fwd(loc, scale, prior4):
    loc = _f32(loc, "loc", 2); scale = _f32(scale, "scale", 2)
    M, D = loc.shape
    kl = torch.empty((M,), dtype=torch.float32, device=loc.device)
    a, b, c, d = (float(v) for v in prior4)
    _lib.check(lib().air_normal_kl_fwd(_p(loc), _p(scale), a, b, c, d, _p(kl), M, D, _stream()), "air_normal_kl_fwd")
    return kl


def normal_kl_bwd(loc, scale, prior4, dkl_row):
    M, D = loc.shape
    dloc = torch.empty_like(loc); dscale = torch.empty_like(scale)
    a, b, c, d = (float(v) for v in prior4)
    _lib.check(lib().air_normal_kl_bwd(_p(loc), _p(scale), a, b, c, d, _p(_f32(dkl_row, "dkl_row", 1)), _p(dloc),
                                       _p(dscale), M, D, _stream()), "air_normal_kl_bwd")
    return dloc, dscale


def presence_fwd(logit, u, step_bias, explore_eps, discrete, presence_in=None):
    """logit, u: [T,B] -> presence_prob[T,B], presence[T,B]"""
    logit = _f32(logit, "logit", 2); u = _f32(u, "u"); presence_in = _f32(presence_in, "presence_in")
    T, B = logit.shape
    prob = torch.empty_like(logit); pres = torch.empty_like(logit)
    eps = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_presence_fwd(_p(logit), _p(u), _p(presence_in), float(step_bias), eps, int(bool(discrete)),
                                      _p(prob), _p(pres), T, B, _stream()), "air_presence_fwd")
    return prob, pres


def presence_bwd(logit, step_bias, explore_eps, discrete, dprob, dpres=None):
    logit = _f32(logit, "logit", 2)
    T, B = logit.shape
    dlogit = torch.empty_like(logit)
    eps = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_presence_bwd(_p(logit), float(step_bias), eps, int(bool(discrete)), _p(_f32(dprob, "dprob")),
                                      _p(_f32(dpres, "dpres")), _p(dlogit), T, B, _stream()), "air_presence_bwd")
    return dlogit


# ---- objective -----------------------------------------------------------------------------------------------------
def rec_loglik_fwd(obs, canvas, mult, std):
    obs = _f32(obs, "obs"); canvas = _f32(canvas, "canvas")
    B = obs.shape[0]
    P = obs.numel() // B
    out = torch.empty((B,), dtype=torch.float32, device=obs.device)
    _lib.check(lib().air_rec_loglik_fwd(_p(obs), _p(canvas), float(mult), float(std), _p(out), B, P, _stream()),
               "air_rec_loglik_fwd")
    return out


def rec_loglik_bwd(obs, canvas, mult, std, dper_sample=None, scale=1.0):
    obs = _f32(obs, "obs"); canvas = _f32(canvas, "canvas")
    B = obs.shape[0]
    P = obs.numel() // B
    dc = torch.empty_like(canvas)
    _lib.check(lib().air_rec_loglik_bwd(_p(obs), _p(canvas), float(mult), float(std),
                                        _p(_f32(dper_sample, "dper_sample")), float(scale), _p(dc), B, P, _stream()),
               "air_rec_loglik_bwd")
    return dc


def numsteps_fwd(presence_prob, presence, prior_f64):
    presence_prob = _f32(presence_prob, "presence_prob", 2); presence = _f32(presence, "presence")
    if prior_f64.dtype != torch.float64 or not prior_f64.is_cuda:
        raise _lib.AirHipError("numsteps: prior must be a float64 CUDA tensor")
    T, B = presence_prob.shape
    dev = presence_prob.device
    q = torch.empty((B, T + 1), dtype=torch.float32, device=dev)
    kl = torch.empty((B,), dtype=torch.float32, device=dev)
    logp = torch.empty((B,), dtype=torch.float32, device=dev) if presence is not None else None
    w = torch.empty((T, B), dtype=torch.float32, device=dev)
    _lib.check(lib().air_numsteps_fwd(_p(presence_prob), _p(presence), _p(prior_f64), _p(q), _p(kl), _p(logp), _p(w),
                                      T, B, _stream()), "air_numsteps_fwd")
    return q, kl, logp, w


def numsteps_bwd(presence_prob, presence, prior_f64, kl_scale, dstep_weight=None, dlogp=None):
    presence_prob = _f32(presence_prob, "presence_prob", 2)
    T, B = presence_prob.shape
    dprob = torch.empty_like(presence_prob)
    _lib.check(lib().air_numsteps_bwd(_p(presence_prob), _p(_f32(presence, "presence")), _p(prior_f64),
                                      float(kl_scale), _p(_f32(dstep_weight, "dstep_weight")),
                                      _p(_f32(dlogp, "dlogp")), _p(dprob), T, B, _stream()), "air_numsteps_bwd")
    return dprob


def _prior_f64(prior_f64, T):
    if not torch.is_tensor(prior_f64) or prior_f64.dtype != torch.float64 or not prior_f64.is_cuda:
        raise _lib.AirHipError("numsteps: prior must be a float64 CUDA tensor")
    if prior_f64.numel() < T + 1:
        raise _lib.AirHipError(f"numsteps: prior holds {prior_f64.numel()} entries, T + 1 = {T + 1} are read")
    return prior_f64


def _tb(shape, **tensors):
    """every given tensor is [T, B] (or [B] when 1-D): the kernels index them by t * B + b without a bound of their own"""
    for nm, t in tensors.items():
        if t is not None and tuple(t.shape) != (tuple(shape) if t.dim() == 2 else (shape[1],)):
            raise _lib.AirHipError(f"{nm}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _numsteps_outputs(T, B, dev):
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    return e(T, B), e(T, B), e(B, T + 1), e(B), e(B), e(T, B)       # prob, presence, q, kl, logp, step weight


def presence_numsteps_fwd(logit, u, step_bias, explore_eps, prior_f64):
    """air_presence_numsteps_fwd: logit[T,B], u[T,B] (None: continuous steps, presence = presence_prob)
    -> presence_prob, presence, q[B,T+1], kl_per_sample[B], logp[B], step_weight[T,B]"""
    logit = _f32(logit, "logit", 2); u = _f32(u, "u", 2)
    T, B = logit.shape
    _tb((T, B), u=u)
    prior_f64 = _prior_f64(prior_f64, T)
    prob, pres, q, kl, logp, w = _numsteps_outputs(T, B, logit.device)
    eps = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_presence_numsteps_fwd(_p(logit), _p(u), float(step_bias), eps, _p(prior_f64), _p(prob), _p(pres),
                                               _p(q), _p(kl), _p(logp), _p(w), T, B, _stream()), "air_presence_numsteps_fwd")
    return prob, pres, q, kl, logp, w


def numsteps_presence_bwd(presence_prob, presence, prior_f64, kl_scale, kl_row_a, kl_row_b, w_scale, dlogp, dpresence, logit,
                          step_bias, explore_eps):
    """air_numsteps_presence_bwd -> dlogit[T,B]; kl_row_a / kl_row_b / dlogp / dpresence may be None"""
    presence_prob = _f32(presence_prob, "presence_prob", 2); logit = _f32(logit, "logit", 2)
    T, B = presence_prob.shape
    _tb((T, B), presence=presence, kl_row_a=kl_row_a, kl_row_b=kl_row_b, dlogp=dlogp, dpresence=dpresence, logit=logit)
    prior_f64 = _prior_f64(prior_f64, T)
    dlogit = torch.empty_like(logit)
    eps = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_numsteps_presence_bwd(_p(presence_prob), _p(_f32(presence, "presence", 2)), _p(prior_f64), float(kl_scale),
                                               _p(_f32(kl_row_a, "kl_row_a", 2)), _p(_f32(kl_row_b, "kl_row_b", 2)), float(w_scale),
                                               _p(_f32(dlogp, "dlogp", 1)), _p(_f32(dpresence, "dpresence", 2)), _p(logit),
                                               float(step_bias), eps, _p(dlogit), T, B, _stream()), "air_numsteps_presence_bwd")
    return dlogit


def _gauss_pre(pre, name):
    if not (torch.is_tensor(pre) and pre.is_cuda and pre.dtype == torch.float32 and pre.dim() == 2 and pre.stride(1) == 1):
        raise _lib.AirHipError(f"{name}: pre must be a 2-D float32 CUDA tensor with unit inner stride")
    return pre.stride(0) if pre.shape[0] > 1 else pre.shape[1]


def heads_fwd(pre, eps, raw_offset, loc_mode, prior4, logit, u, step_bias, explore_eps, prior_f64, guard_eps=0.0):
    """air_heads_fwd = gauss_sample_fwd(pre, eps, ...) || presence_numsteps_fwd(logit, u, ...) in one launch
    -> (loc, scale, sample, kl_row), (presence_prob, presence, q, kl_per_sample, logp, step_weight)"""
    ld = _gauss_pre(pre, "heads_fwd")
    eps = _f32(eps, "eps", 2); logit = _f32(logit, "logit", 2); u = _f32(u, "u", 2)
    M, D = eps.shape
    T, B = logit.shape
    _tb((T, B), u=u)
    if pre.shape[0] != M or pre.shape[1] < 2 * D:
        raise _lib.AirHipError(f"heads_fwd: pre is {tuple(pre.shape)}, eps {tuple(eps.shape)}")
    prior_f64 = _prior_f64(prior_f64, T)
    dev = pre.device
    loc = torch.empty((M, D), dtype=torch.float32, device=dev); scale = torch.empty_like(loc); sample = torch.empty_like(loc)
    kl_row = torch.empty((M,), dtype=torch.float32, device=dev)
    prob, pres, q, kl, logp, w = _numsteps_outputs(T, B, dev)
    a, b, c, d = (float(v) for v in prior4)
    xe = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_heads_fwd(_p(pre), ld, _p(eps), float(raw_offset), int(loc_mode), a, b, c, d, _p(loc), _p(scale),
                                   _p(sample), _p(kl_row), M, D, _p(logit), _p(u), float(step_bias), xe, _p(prior_f64),
                                   _p(prob), _p(pres), _p(q), _p(kl), _p(logp), _p(w), T, B, float(guard_eps), _stream()),
               "air_heads_fwd")
    return (loc, scale, sample, kl_row), (prob, pres, q, kl, logp, w)


def heads_bwd(pre, eps, raw_offset, loc_mode, prior4, loc, scale, dsample, dkl_row, presence_prob, presence, prior_f64,
              kl_scale, kl_row_a, kl_row_b, w_scale, dlogp, dpresence, logit, step_bias, explore_eps, guard_eps=0.0):
    """air_heads_bwd = gauss_sample_bwd || numsteps_presence_bwd in one launch -> dpre[M,2D], dlogit[T,B]"""
    ld = _gauss_pre(pre, "heads_bwd")
    loc = _f32(loc, "loc", 2); scale = _f32(scale, "scale", 2); eps = _f32(eps, "eps", 2)
    presence_prob = _f32(presence_prob, "presence_prob", 2); logit = _f32(logit, "logit", 2)
    M, D = loc.shape
    T, B = presence_prob.shape
    _tb((T, B), presence=presence, kl_row_a=kl_row_a, kl_row_b=kl_row_b, dlogp=dlogp, dpresence=dpresence, logit=logit)
    _tb((M, D), scale=scale, eps=eps, dsample=dsample)
    if pre.shape[0] != M or pre.shape[1] < 2 * D or (dkl_row is not None and tuple(dkl_row.shape) != (M,)):
        raise _lib.AirHipError(f"heads_bwd: pre is {tuple(pre.shape)}, loc {tuple(loc.shape)}")
    prior_f64 = _prior_f64(prior_f64, T)
    dpre = torch.empty((M, 2 * D), dtype=torch.float32, device=pre.device)
    dlogit = torch.empty_like(logit)
    a, b, c, d = (float(v) for v in prior4)
    xe = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_heads_bwd(_p(pre), ld, _p(eps), float(raw_offset), int(loc_mode), a, b, c, d, _p(loc), _p(scale),
                                   _p(_f32(dsample, "dsample", 2)), None, _p(_f32(dkl_row, "dkl_row", 1)), 1.0, _p(dpre), 2 * D,
                                   M, D, _p(presence_prob), _p(_f32(presence, "presence", 2)), _p(prior_f64), float(kl_scale),
                                   _p(_f32(kl_row_a, "kl_row_a", 2)), _p(_f32(kl_row_b, "kl_row_b", 2)), float(w_scale),
                                   _p(_f32(dlogp, "dlogp", 1)), _p(_f32(dpresence, "dpresence", 2)), _p(logit), float(step_bias),
                                   xe, _p(dlogit), T, B, float(guard_eps), _stream()), "air_heads_bwd")
    return dpre, dlogit


ANNEAL_TYPES = {None: 0, "exp": 1, "linear": 2}


def steps_prior(global_step_dev, T, init, final_value=0.0, anneal_type=None, anneal_steps=1.0, hold_for=0.0, steps_div=1.0):
    """air_steps_prior: the annealed geometric prior table [T+1] (float64, not renormalised) at the step count held on the
    device in global_step_dev (an int64 CUDA tensor of one element)."""
    if not (torch.is_tensor(global_step_dev) and global_step_dev.is_cuda and global_step_dev.dtype == torch.int64
            and global_step_dev.numel() >= 1):
        raise _lib.AirHipError("steps_prior: global_step_dev must be an int64 CUDA tensor")
    if anneal_type not in ANNEAL_TYPES:
        raise _lib.AirHipError(f"steps_prior: anneal_type must be one of {list(ANNEAL_TYPES)}")
    out = torch.empty((int(T) + 1,), dtype=torch.float64, device=global_step_dev.device)
    _lib.check(lib().air_steps_prior(_p(global_step_dev), ANNEAL_TYPES[anneal_type], float(init), float(final_value),
                                     float(anneal_steps), float(hold_for), float(steps_div), _p(out), int(T), _stream()),
               "air_steps_prior")
    return out


def nvil(imp, baseline, logp, ema=None):
    """ema: None, or the DEVICE block of four floats {moving_mean, moving_var, decay, update} (updated in place when update != 0)"""
    imp = _f32(imp, "imp", 1); baseline = _f32(baseline, "baseline", 1); logp = _f32(logp, "logp", 1)
    ema = _f32(ema, "ema", 1)
    if ema is not None and ema.numel() != 4:
        raise _lib.AirHipError("nvil: ema must hold four floats {moving_mean, moving_var, decay, update}")
    B = imp.shape[0]
    dev = imp.device
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    dlogp = torch.empty((B,), dtype=torch.float32, device=dev); dbase = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.check(lib().air_nvil(_p(imp), _p(baseline), _p(logp), _p(out), _p(dlogp), _p(dbase), B, _p(ema), _stream()), "air_nvil")
    return out, dlogp, dbase


def _iw_rows(what, what_loc, what_scale, where, where_loc, where_scale, presence, K):
    """shapes behind air_iw_logweight / air_iw_logweight_bwd: what-like [T,R,A], where-like [T,R,4], presence [T,R] (or [T,R,1])"""
    what = _f32(what, "what", 3)
    T, R, A = what.shape
    for t, nm in ((what_loc, "what_loc"), (what_scale, "what_scale")):
        if tuple(_f32(t, nm, 3).shape) != (T, R, A):
            raise _lib.AirHipError(f"{nm}: expected shape {(T, R, A)}, got {tuple(t.shape)}")
    for t, nm in ((where, "where"), (where_loc, "where_loc"), (where_scale, "where_scale")):
        if tuple(_f32(t, nm, 3).shape) != (T, R, 4):
            raise _lib.AirHipError(f"{nm}: expected shape {(T, R, 4)}, got {tuple(t.shape)}")
    if _f32(presence, "presence").numel() != T * R:
        raise _lib.AirHipError(f"presence: expected {T * R} entries, got shape {tuple(presence.shape)}")
    if int(K) < 1 or R % int(K):
        raise _lib.AirHipError(f"K = {K} does not divide the {R} rows")
    return T, R, A


def _iw_row_vec(t, name, R):
    if _f32(t, name, 1).shape[0] != R:
        raise _lib.AirHipError(f"{name}: expected {R} entries, got shape {tuple(t.shape)}")
    return t


def iw_logweight(what, what_loc, what_scale, where, where_loc, where_scale, presence, rec, logp, prior_f64, K, priors6, normalize=False):
    """air_iw_logweight: -> logw[R], num_steps[R] (int32).  priors6 = (what loc, scale, where-scale loc, scale, where-shift loc, scale),
    the shift loc NaN for a prior centred on where_loc."""
    T, R, A = _iw_rows(what, what_loc, what_scale, where, where_loc, where_scale, presence, K)
    _iw_row_vec(rec, "rec", R); _iw_row_vec(logp, "logp", R)
    prior_f64 = _prior_f64(prior_f64, T)
    logw = torch.empty((R,), dtype=torch.float32, device=what.device)
    n = torch.empty((R,), dtype=torch.int32, device=what.device)
    pr = [float(v) for v in priors6]
    _lib.check(lib().air_iw_logweight(_p(what), _p(what_loc), _p(what_scale), _p(where), _p(where_loc), _p(where_scale), _p(presence),
                                      _p(rec), _p(logp), _p(prior_f64), T, R, int(K), A, *pr, 1 if normalize else 0, _p(logw), _p(n),
                                      _stream()), "air_iw_logweight")
    return logw, n


def iw_logweight_bwd(what, what_loc, what_scale, where, where_loc, where_scale, presence, g, K, priors6):
    """air_iw_logweight_bwd: -> d what, d what_loc, d what_scale [T,R,A], d where, d where_loc, d where_scale [T,R,4], d rec [R], d logp [R]"""
    T, R, A = _iw_rows(what, what_loc, what_scale, where, where_loc, where_scale, presence, K)
    _iw_row_vec(g, "g", R)
    outs = [torch.empty_like(what) for _ in range(3)] + [torch.empty_like(where) for _ in range(3)] + \
           [torch.empty((R,), dtype=torch.float32, device=what.device) for _ in range(2)]
    pr = [float(v) for v in priors6]
    _lib.check(lib().air_iw_logweight_bwd(_p(what), _p(what_loc), _p(what_scale), _p(where), _p(where_loc), _p(where_scale),
                                          _p(presence), _p(g), T, R, int(K), A, *pr, *[_p(o) for o in outs], _stream()),
               "air_iw_logweight_bwd")
    return tuple(outs)


def iw_vimco(logw, K):
    """air_iw_vimco: logw[R] (R = B * K, row b * K + k) -> bound[B], wnorm[R], signal[R], ess[B], degenerate[B] (int32)"""
    logw = _f32(logw, "logw", 1)
    R, K = logw.shape[0], int(K)
    if K < 2 or R == 0 or R % K:
        raise _lib.AirHipError(f"iw_vimco: K = {K} must be >= 2 and divide the {R} rows")
    dev = logw.device
    B = R // K
    e = lambda n, dt=torch.float32: torch.empty((n,), dtype=dt, device=dev)
    bound, wnorm, signal, ess, degen = e(B), e(R), e(R), e(B), e(B, torch.int32)
    _lib.check(lib().air_iw_vimco(_p(logw), R, K, _p(bound), _p(wnorm), _p(signal), _p(ess), _p(degen), _stream()), "air_iw_vimco")
    return bound, wnorm, signal, ess, degen


def iw_logposterior(what, what_loc, what_scale, where, where_loc, where_scale, presence, logp, K):
    """air_iw_logposterior: -> log_q[R] = logp + sum_{t<n} log N(what_t | .) + log N(where_t | .) (with the -1/2 log 2 pi of every term)"""
    T, R, A = _iw_rows(what, what_loc, what_scale, where, where_loc, where_scale, presence, K)
    _iw_row_vec(logp, "logp", R)
    log_q = torch.empty((R,), dtype=torch.float32, device=what.device)
    _lib.check(lib().air_iw_logposterior(_p(what), _p(what_loc), _p(what_scale), _p(where), _p(where_loc), _p(where_scale),
                                         _p(presence), _p(logp), T, R, int(K), A, _p(log_q), _stream()), "air_iw_logposterior")
    return log_q


def iw_logposterior_bwd(what, what_loc, what_scale, where, where_loc, where_scale, presence, g, K, want_what=True, want_where=True):
    """air_iw_logposterior_bwd: -> d what (None without want_what), d what_loc, d what_scale [T,R,A], d where (None without
    want_where), d where_loc, d where_scale [T,R,4], d logp [R]"""
    T, R, A = _iw_rows(what, what_loc, what_scale, where, where_loc, where_scale, presence, K)
    _iw_row_vec(g, "g", R)
    outs = [torch.empty_like(what) if want_what else None, torch.empty_like(what), torch.empty_like(what),
            torch.empty_like(where) if want_where else None, torch.empty_like(where), torch.empty_like(where),
            torch.empty((R,), dtype=torch.float32, device=what.device)]
    _lib.check(lib().air_iw_logposterior_bwd(_p(what), _p(what_loc), _p(what_scale), _p(where), _p(where_loc), _p(where_scale),
                                             _p(presence), _p(g), T, R, int(K), A, *[_p(o) for o in outs], _stream()),
               "air_iw_logposterior_bwd")
    return tuple(outs)


def nvil_parts(imp_parts, baseline, logp, ema=None, want_sum=True):
    """air_nvil_parts: imp_parts[n_parts, B] shares of the importance weight -> out[4], dlogp[B], dbaseline[B], imp_sum[B] | None"""
    imp_parts = _f32(imp_parts, "imp_parts", 2); baseline = _f32(baseline, "baseline", 1); logp = _f32(logp, "logp", 1)
    ema = _f32(ema, "ema", 1)
    if ema is not None and ema.numel() != 4:
        raise _lib.AirHipError("nvil_parts: ema must hold four floats {moving_mean, moving_var, decay, update}")
    n_parts, B = imp_parts.shape
    if baseline.shape[0] != B or logp.shape[0] != B:
        raise _lib.AirHipError("nvil_parts: baseline / logp must hold B entries")
    dev = imp_parts.device
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    dlogp = torch.empty((B,), dtype=torch.float32, device=dev); dbase = torch.empty((B,), dtype=torch.float32, device=dev)
    imp_sum = torch.empty((B,), dtype=torch.float32, device=dev) if want_sum else None
    _lib.check(lib().air_nvil_parts(_p(imp_parts), n_parts, _p(imp_sum), _p(baseline), _p(logp), _p(out), _p(dlogp), _p(dbase),
                                    B, _p(ema), _stream()), "air_nvil_parts")
    return out, dlogp, dbase, imp_sum


def imp_weight(rec_parts, step_weight, kl_n=None, nsp_weight=1.0, kl_row_a=None, kl_row_b=None, want_imp=True,
               dpresence_inout=None, dkl_scale=0.0, want_rec=True):
    """air_imp_weight: rec_parts[n_parts,B], step_weight[T,B] -> rec[B] | None, imp[B] | None;
    dpresence_inout[T,B] (optional) += dkl_scale * (kl_row_a + kl_row_b) in place."""
    rec_parts = _f32(rec_parts, "rec_parts", 2); step_weight = _f32(step_weight, "step_weight", 2)
    n_parts, B = rec_parts.shape
    T = step_weight.shape[0]
    for t, nm in ((kl_row_a, "kl_row_a"), (kl_row_b, "kl_row_b"), (dpresence_inout, "dpresence_inout")):
        _f32(t, nm, 2)
    _tb((T, B), step_weight=step_weight, kl_n=_f32(kl_n, "kl_n", 1), kl_row_a=kl_row_a, kl_row_b=kl_row_b,
        dpresence_inout=dpresence_inout)
    if not want_imp and dpresence_inout is None:
        raise _lib.AirHipError("imp_weight: one of imp / dpresence_inout is required")
    dev = rec_parts.device
    rec = torch.empty((B,), dtype=torch.float32, device=dev) if want_rec else None
    imp = torch.empty((B,), dtype=torch.float32, device=dev) if want_imp else None
    _lib.check(lib().air_imp_weight(_p(rec_parts), n_parts, _p(rec), _p(_f32(kl_n, "kl_n", 1)), float(nsp_weight), _p(kl_row_a),
                                    _p(kl_row_b), _p(step_weight), T, B, _p(imp), _p(dpresence_inout), float(dkl_scale),
                                    _stream()), "air_imp_weight")
    return rec, imp


def baseline_pack(img, what, where, presence, state_parts):
    """img[B,...], what[T,B,A], where[T,B,4], presence[T,B(,1)], state_parts: list of up to two [B,S] tensors."""
    img = _f32(img, "img"); what = _f32(what, "what", 3); where = _f32(where, "where", 3)
    presence = _f32(presence, "presence")
    T, B, A = what.shape
    Pn = img.numel() // B
    parts = [_f32(s, "state", 2) for s in state_parts]
    if len(parts) > 2:
        raise _lib.AirHipError("baseline_pack: at most two state parts")
    s0 = parts[0] if len(parts) > 0 else None
    s1 = parts[1] if len(parts) > 1 else None
    S0 = s0.shape[1] if s0 is not None else 0
    S1 = s1.shape[1] if s1 is not None else 0
    out = torch.empty((B, Pn + T * A + T * 4 + T + S0 + S1), dtype=torch.float32, device=img.device)
    _lib.check(lib().air_baseline_pack(_p(img), _p(what), _p(where), _p(presence), _p(s0), _p(s1), _p(out), T, B, Pn,
                                       A, S0, S1, _stream()), "air_baseline_pack")
    return out


# ---- the fused launches around the glimpse read, the `what` head ---------------------------------------------------
def _nan(*shape, device):
    """an output buffer filled with NaN: an element the launch leaves out shows up in the caller's comparison"""
    return torch.full(shape, float("nan"), dtype=torch.float32, device=device)


def _mat(t, name, cols=None):
    """a 2-D float32 CUDA tensor with unit inner stride (a row view of a wider buffer is fine) -> its leading dimension"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
        raise _lib.AirHipError(f"{name}: expected a 2-D float32 CUDA tensor with unit inner stride")
    if cols is not None and t.shape[1] != cols:
        raise _lib.AirHipError(f"{name}: expected {cols} columns, got shape {tuple(t.shape)}")
    return max(t.stride(0), t.shape[1])                         # (a single row keeps the stride of the buffer it was cut from)


def attend_fwd(tr_h, tr_w, tr_b, st_h, st_w, st_b, eps, raw_offset, prior4, u, step_bias, explore_eps, prior_f64, img, crop_size,
               precision=0, guard_eps=0.0):
    """air_attend_fwd: tr_h[T*B, tr_k], tr_w[tr_k, 8], tr_b[8], st_h[T*B, st_k], st_w[st_k], st_b[1], eps[T*B, 4], u[T, B] | None,
    img[B, H, W] -> (pre[T*B, 8], logit[T, B]), (loc, scale, where [T*B, 4], kl_row[T*B]),
    (presence_prob, presence, q[B, T+1], kl_per_sample[B], logp[B], step_weight[T, B]), glimpse[T*B, h, w]"""
    tr_h = _f32(tr_h, "tr_h", 2); tr_w = _f32(tr_w, "tr_w", 2); tr_b = _f32(tr_b, "tr_b", 1)
    st_h = _f32(st_h, "st_h", 2); st_w = _f32(st_w, "st_w"); st_b = _f32(st_b, "st_b", 1)
    eps = _f32(eps, "eps", 2); img = _f32(img, "img", 3); u = _f32(u, "u", 2)
    B, H, W = img.shape
    M, tr_k = tr_h.shape
    st_k = st_h.shape[1]
    T = M // B
    if T * B != M or st_h.shape[0] != M or tuple(eps.shape) != (M, 4) or tuple(tr_w.shape) != (tr_k, 8) or tr_b.numel() != 8 \
            or st_w.numel() != st_k or st_b.numel() != 1:
        raise _lib.AirHipError(f"attend_fwd: tr_h {tuple(tr_h.shape)}, tr_w {tuple(tr_w.shape)}, st_h {tuple(st_h.shape)}, st_w "
                               f"{tuple(st_w.shape)}, eps {tuple(eps.shape)} for {B} images")
    _tb((T, B), u=u)
    prior_f64 = _prior_f64(prior_f64, T)
    h, w = int(crop_size[0]), int(crop_size[1])
    dev = img.device
    pre = _nan(M, 8, device=dev); logit = _nan(T, B, device=dev)
    loc, scale, where = (_nan(M, 4, device=dev) for _ in range(3))
    kl_row = _nan(M, device=dev)
    prob, pres, step_w = (_nan(T, B, device=dev) for _ in range(3))
    q = _nan(B, T + 1, device=dev); kl = _nan(B, device=dev); logp = _nan(B, device=dev)
    glimpse = _nan(M, h, w, device=dev)
    a, b, c, d = (float(v) for v in prior4)
    xe = -1.0 if explore_eps is None else float(explore_eps)
    _lib.check(lib().air_attend_fwd(_p(tr_h), _p(tr_w), _p(tr_b), tr_k, _p(st_h), _p(st_w), _p(st_b), st_k, _p(pre), _p(logit), _p(eps),
                                    float(raw_offset), a, b, c, d, _p(loc), _p(scale), _p(where), _p(kl_row), _p(u), float(step_bias), xe,
                                    _p(prior_f64), _p(prob), _p(pres), _p(q), _p(kl), _p(logp), _p(step_w), _p(img), _p(glimpse),
                                    T, B, H, W, h, w, int(precision), float(guard_eps), _stream()), "air_attend_fwd")
    return (pre, logit), (loc, scale, where, kl_row), (prob, pres, q, kl, logp, step_w), glimpse


def attend_bwd(img, where, dglimpse, pre, eps, raw_offset, prior4, loc, scale, dwhere_w, dkl_row, dkl_scale, presence_prob, presence,
               prior_f64, kl_scale, kl_row_a, kl_row_b, w_scale, dlogp, dpresence, logit, step_bias, explore_eps, guard_eps=0.0,
               tr_w=None, tr_y=None, tr_dx=None, st_w=None, st_y=None, st_dx=None, precision=0):
    """air_attend_bwd -> dwhere_r[T*B, 4], dpre[T*B, 8], dlogit[T, B].  dwhere_w[slabs, T*B, 4] (1..4 slabs); dkl_row, kl_row_a,
    kl_row_b, dlogp, dpresence may be None.
    With tr_w[tr_k, 8] and st_w[st_k] given: air_attend_bwd_dx, which also returns tr_dx[T*B, tr_k] and st_dx[T*B, st_k].  tr_y / st_y
    (or None) and tr_dx / st_dx (or None: allocated here) may be row views of wider buffers, all of one leading dimension per layer."""
    img = _f32(img, "img", 3); where = _f32(where, "where", 2); dglimpse = _f32(dglimpse, "dglimpse", 3)
    pre = _f32(pre, "pre", 2); eps = _f32(eps, "eps", 2); loc = _f32(loc, "loc", 2); scale = _f32(scale, "scale", 2)
    dwhere_w = _f32(dwhere_w, "dwhere_w", 3); dkl_row = _f32(dkl_row, "dkl_row", 1)
    presence_prob = _f32(presence_prob, "presence_prob", 2); logit = _f32(logit, "logit", 2)
    B, H, W = img.shape
    M, h, w = dglimpse.shape
    T = presence_prob.shape[0]
    if T * B != M or presence_prob.shape[1] != B or tuple(pre.shape) != (M, 8) or tuple(dwhere_w.shape[1:]) != (M, 4) \
            or (dkl_row is not None and dkl_row.shape[0] != M):
        raise _lib.AirHipError(f"attend_bwd: dglimpse {tuple(dglimpse.shape)}, pre {tuple(pre.shape)}, dwhere_w {tuple(dwhere_w.shape)}, "
                               f"presence_prob {tuple(presence_prob.shape)} for {B} images")
    _tb((M, 4), where=where, eps=eps, loc=loc, scale=scale)
    _tb((T, B), presence=_f32(presence, "presence", 2), kl_row_a=_f32(kl_row_a, "kl_row_a", 2), kl_row_b=_f32(kl_row_b, "kl_row_b", 2),
        dlogp=_f32(dlogp, "dlogp", 1), dpresence=_f32(dpresence, "dpresence", 2), logit=logit)
    prior_f64 = _prior_f64(prior_f64, T)
    dev = img.device
    dwhere_r = _nan(M, 4, device=dev); dpre = _nan(M, 8, device=dev); dlogit = _nan(T, B, device=dev)
    a, b, c, d = (float(v) for v in prior4)
    xe = -1.0 if explore_eps is None else float(explore_eps)
    head = (_p(img), _p(where), _p(dglimpse), _p(dwhere_r), _p(pre), _p(eps), float(raw_offset), a, b, c, d, _p(loc), _p(scale),
            _p(dwhere_w), int(dwhere_w.shape[0]), _p(dkl_row), float(dkl_scale), _p(dpre), _p(presence_prob), _p(presence), _p(prior_f64),
            float(kl_scale), _p(kl_row_a), _p(kl_row_b), float(w_scale), _p(dlogp), _p(dpresence), _p(logit), float(step_bias), xe,
            _p(dlogit), T, B, H, W, h, w)
    if tr_w is None and st_w is None:
        _lib.check(lib().air_attend_bwd(*head, float(guard_eps), _stream()), "air_attend_bwd")
        return dwhere_r, dpre, dlogit
    tr_w = _f32(tr_w, "tr_w", 2); st_w = _f32(st_w, "st_w")
    tr_k, st_k = tr_w.shape[0], st_w.numel()
    if tr_dx is None:
        tr_dx = _nan(M, tr_k, device=dev)
    if st_dx is None:
        st_dx = _nan(M, st_k, device=dev)
    tr_ld, st_ld = _mat(tr_dx, "tr_dx", tr_k), _mat(st_dx, "st_dx", st_k)
    for y, ld, k, nm in ((tr_y, tr_ld, tr_k, "tr_y"), (st_y, st_ld, st_k, "st_y")):
        if y is not None and (_mat(y, nm, k) != ld or y.shape[0] != M):
            raise _lib.AirHipError(f"attend_bwd: {nm} must hold {M} rows of the leading dimension of its dx ({ld})")
    if tr_dx.shape[0] != M or st_dx.shape[0] != M or tr_w.shape[1] != 8:
        raise _lib.AirHipError(f"attend_bwd: tr_dx {tuple(tr_dx.shape)}, st_dx {tuple(st_dx.shape)}, tr_w {tuple(tr_w.shape)}")
    _lib.check(lib().air_attend_bwd_dx(*head, _p(tr_w), _p(tr_y), _p(tr_dx), tr_k, tr_ld, _p(st_w), _p(st_y), _p(st_dx), st_k, st_ld,
                                       int(precision), float(guard_eps), _stream()), "air_attend_bwd_dx")
    return dwhere_r, dpre, dlogit, tr_dx, st_dx


def _what_pack_args(where, presence, state_parts, T, B):
    where = _f32(where, "where", 3); presence = _f32(presence, "presence")
    parts = [_f32(s, "state", 2) for s in state_parts]
    if len(parts) > 2 or tuple(where.shape) != (T, B, 4) or presence.numel() != T * B or any(s.shape[0] != B for s in parts):
        raise _lib.AirHipError(f"what head: where {tuple(where.shape)}, presence {tuple(presence.shape)}, {len(parts)} state parts")
    s0 = parts[0] if len(parts) > 0 else None
    s1 = parts[1] if len(parts) > 1 else None
    return where, presence, s0, s1, (s0.shape[1] if s0 is not None else 0), (s1.shape[1] if s1 is not None else 0)


def what_head_fwd(x, w, b, eps, raw_offset, prior2, where, presence, state_parts, T, precision=0, guard_eps=0.0):
    """air_what_head_fwd: x[T*B, K] (a row view is fine), w[K, 2A], b[2A], eps[T*B, A], where[T, B, 4], presence[T, B], up to two
    state parts [B, S] -> q[T*B, 2A], loc, scale, sample [T*B, A], kl_parts[ceil(A / 8), T*B], pack_out[B, T*A + 5T + S0 + S1]"""
    ldx = _mat(x, "x")
    w = _f32(w, "w", 2); b = _f32(b, "b", 1); eps = _f32(eps, "eps", 2)
    M, K = x.shape
    A = w.shape[1] // 2
    B = M // int(T)
    if B * T != M or tuple(w.shape) != (K, 2 * A) or b.numel() != 2 * A or tuple(eps.shape) != (M, A):
        raise _lib.AirHipError(f"what_head_fwd: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}, eps {tuple(eps.shape)}, T {T}")
    where, presence, s0, s1, S0, S1 = _what_pack_args(where, presence, state_parts, T, B)
    dev = x.device
    q = _nan(M, 2 * A, device=dev)
    loc, scale, sample = (_nan(M, A, device=dev) for _ in range(3))
    kl_parts = _nan(int(lib().air_what_head_parts(A)), M, device=dev)
    pack = _nan(B, T * A + 5 * T + S0 + S1, device=dev)
    _lib.check(lib().air_what_head_fwd(_p(x), ldx, K, _p(w), _p(b), _p(eps), float(raw_offset), float(prior2[0]), float(prior2[1]), _p(q),
                                       _p(loc), _p(scale), _p(sample), _p(kl_parts), A, _p(where), _p(presence), _p(s0), _p(s1), _p(pack),
                                       int(T), B, S0, S1, float(guard_eps), int(precision), _stream()), "air_what_head_fwd")
    return q, loc, scale, sample, kl_parts, pack


def what_sample_pack(pre, eps, raw_offset, prior2, where, presence, state_parts, T, guard_eps=0.0):
    """air_what_sample_pack: pre[T*B, >= 2A] (row stride allowed), eps[T*B, A] -> loc, scale, sample [T*B, A], kl_row[T*B],
    pack_out[B, T*A + 5T + S0 + S1]"""
    ld = _mat(pre, "pre")
    eps = _f32(eps, "eps", 2)
    M, A = eps.shape
    B = M // int(T)
    if B * T != M or pre.shape[0] != M or pre.shape[1] < 2 * A:
        raise _lib.AirHipError(f"what_sample_pack: pre {tuple(pre.shape)}, eps {tuple(eps.shape)}, T {T}")
    where, presence, s0, s1, S0, S1 = _what_pack_args(where, presence, state_parts, T, B)
    dev = pre.device
    loc, scale, sample = (_nan(M, A, device=dev) for _ in range(3))
    kl_row = _nan(M, device=dev)
    pack = _nan(B, T * A + 5 * T + S0 + S1, device=dev)
    _lib.check(lib().air_what_sample_pack(_p(pre), ld, _p(eps), float(raw_offset), float(prior2[0]), float(prior2[1]), _p(loc), _p(scale),
                                          _p(sample), _p(kl_row), A, _p(where), _p(presence), _p(s0), _p(s1), _p(pack), int(T), B, S0, S1,
                                          float(guard_eps), _stream()), "air_what_sample_pack")
    return loc, scale, sample, kl_row, pack


# ---- optimiser / noise / utils -------------------------------------------------------------------------------------
def rmsprop_centered_(p, g, ms, mg, mom, lr_dev, lr_mult=1.0, decay=0.9, momentum=0.9, eps=1e-10, grad_scale=1.0,
                      centered=True):
    """tf.train.RMSPropOptimizer's update (all of its keywords) in place; `centered=True, momentum=.9` is the reference's
    choice (model.py:265)."""
    for t, nm in ((p, "p"), (g, "g"), (ms, "ms"), (mg, "mg"), (mom, "mom"), (lr_dev, "lr_dev")):
        _f32(t, nm)
    _lib.check(lib().air_rmsprop(_p(p), _p(g), _p(ms), _p(mg), _p(mom), ctypes.c_size_t(p.numel()), _p(lr_dev),
                                 float(lr_mult), float(decay), float(momentum), float(eps), int(bool(centered)),
                                 float(grad_scale), _stream()), "air_rmsprop")


def rng_fill(state_dev, normal=None, uniform=None, advance=True):
    """state_dev: int64/uint64 CUDA tensor [2] = {seed, offset}.  Fills the given flat tensors in place."""
    nn = normal.numel() if normal is not None else 0
    nu = uniform.numel() if uniform is not None else 0
    _lib.check(lib().air_rng_fill(_p(normal), ctypes.c_size_t(nn), _p(uniform), ctypes.c_size_t(nu), _p(state_dev),
                                  _stream()), "air_rng_fill")
    if advance:
        _lib.check(lib().air_rng_advance(_p(state_dev), ctypes.c_uint64((nn + 3) // 4 + (nu + 3) // 4), _stream()),
                   "air_rng_advance")


def fill_(t, v):
    _lib.check(lib().air_fill(_p(t), ctypes.c_size_t(t.numel()), float(v), _stream()), "air_fill")
    return t


def axpby(a, alpha, b=None, beta=0.0, out=None):
    out = torch.empty_like(a) if out is None else out
    _lib.check(lib().air_axpby(_p(a), float(alpha), _p(b), float(beta), _p(out), ctypes.c_size_t(a.numel()),
                               _stream()), "air_axpby")
    return out


def tile_rows(src, rows):
    src = _f32(src, "src")
    cols = src.numel()
    out = torch.empty((rows, cols), dtype=torch.float32, device=src.device)
    _lib.check(lib().air_tile_rows(_p(src), _p(out), rows, cols, _stream()), "air_tile_rows")
    return out


def colsum(x):
    M, N = x.shape
    out = torch.empty((N,), dtype=torch.float32, device=x.device)
    _lib.check(lib().air_colsum(_p(x), x.stride(0) if M > 1 else N, _p(out), M, N, _stream()), "air_colsum")
    return out


# ---- the folded launches of the train step (tests/test_fold_kernels.py calls each on its own) --------------------------------------
E_UNSUPPORTED = -5                                                      # AIR_E_UNSUPPORTED: a launch declines a shape it has no form for


def _status(st, what):
    """0, or AIR_E_UNSUPPORTED handed back as the integer it is (a decline is an answer, the caller plans the unfused launches);
    anything else raises"""
    if st != E_UNSUPPORTED:
        _lib.check(st, what)
    return int(st)


def _i64(t, name, n=1):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.int64, getattr(torch, "uint64", torch.int64)) and t.numel() >= n):
        raise _lib.AirHipError(f"{name}: expected an int64 CUDA tensor of at least {n} element(s)")
    return t


def step_epilogue_(p, g, ms, mg, mom, n_model, lr_dev, lr_mult_tail=1.0, decay=0.9, momentum=0.9, eps=1e-10, grad_scale=1.0,
                   global_step_dev=None, rng_state_dev=None, rng_increment=0):
    """air_step_epilogue over p.numel() elements, in place (elements >= n_model use lr * lr_mult_tail); the counters advance when given"""
    for t, nm in ((p, "p"), (g, "g"), (ms, "ms"), (mg, "mg"), (mom, "mom"), (lr_dev, "lr_dev")):
        _f32(t, nm)
    _lib.check(lib().air_step_epilogue(_p(p), _p(g), _p(ms), _p(mg), _p(mom), ctypes.c_size_t(int(n_model)), ctypes.c_size_t(p.numel()),
                                       _p(lr_dev), float(lr_mult_tail), float(decay), float(momentum), float(eps), float(grad_scale),
                                       _p(_i64(global_step_dev, "global_step_dev")), _p(_i64(rng_state_dev, "rng_state_dev", 2)),
                                       ctypes.c_uint64(int(rng_increment)), _stream()), "air_step_epilogue")


def opt_fold(p, g, ms, mg, mom, n_model, lr_dev, fold_mask, ranges=(), lr_mult_tail=1.0, decay=0.9, momentum=0.9, eps=1e-10,
             grad_scale=1.0, global_step_dev=None, rng_state_dev=None, rng_increment=0):
    """AirOptFold over the flat buffers: the problems of fold_mask update where they write, `ranges` = up to four (lo, hi) rider slices"""
    for t, nm in ((p, "p"), (g, "g"), (ms, "ms"), (mg, "mg"), (mom, "mom"), (lr_dev, "lr_dev")):
        _f32(t, nm)
    if len(ranges) > 4:
        raise _lib.AirHipError("opt_fold: at most four rider ranges")
    lo = (ctypes.c_size_t * 4)(*([int(r[0]) for r in ranges] + [0] * (4 - len(ranges))))
    hi = (ctypes.c_size_t * 4)(*([int(r[1]) for r in ranges] + [0] * (4 - len(ranges))))
    gs, rs = _i64(global_step_dev, "global_step_dev"), _i64(rng_state_dev, "rng_state_dev", 2)
    return _lib.AirOptFold(p.data_ptr(), g.data_ptr(), ms.data_ptr(), mg.data_ptr(), mom.data_ptr(), int(n_model), lr_dev.data_ptr(),
                           float(lr_mult_tail), float(decay), float(momentum), float(eps), float(grad_scale), int(fold_mask),
                           len(ranges), lo, hi, gs.data_ptr() if gs is not None else None, rs.data_ptr() if rs is not None else None,
                           int(rng_increment))


def gemm_grouped_opt(problems, opt, precision=0):
    """air_gemm_grouped_opt: problems as for gemm_grouped (a folded problem's `out` / `colsum` are views of the flat gradient buffer),
    opt = opt_fold(...) -> (status, [(C, colsum|None)]); status is 0 or AIR_E_UNSUPPORTED (nothing launched)"""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped_opt")
    st = _status(lib().air_gemm_grouped_opt(arr, len(outs), ctypes.byref(opt), _stream()), "air_gemm_grouped_opt")
    return st, outs


def gemm_grouped_gauss_bwd(problems, problem, pre, eps, raw_offset, prior2, loc, scale, dkl_row, dkl_scale, dpre, guard_eps=0.0,
                           precision=0, nvil=None, kl_parts=None):
    """air_gemm_grouped_gauss_bwd: problem `problem` of the group is dsample[M, D]; pre[M, >= 2D] and dpre[M, >= 2D] may be row views
    (ld_pre, ld_dpre), eps / loc / scale [M, D], dkl_row[M] | None.  nvil: None, or dict(imp_parts[n_parts, B], baseline[B], logp[B],
    ema = the four-float block | None).  kl_parts[n_kl_parts, M] | None.
    -> (status, [(C, colsum|None)], dict(out[4], dlogp[B], dbaseline[B], imp_sum[B], kl_row[M]) of the riders that ran, NaN-primed)"""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped_gauss_bwd")
    ld_pre, ld_dpre = _mat(pre, "pre"), _mat(dpre, "dpre")
    eps = _f32(eps, "eps", 2); loc = _f32(loc, "loc", 2); scale = _f32(scale, "scale", 2); dkl_row = _f32(dkl_row, "dkl_row", 1)
    M, D = eps.shape
    _tb((M, D), loc=loc, scale=scale)
    if pre.shape[0] != M or dpre.shape[0] != M or pre.shape[1] < 2 * D or dpre.shape[1] < 2 * D or (dkl_row is not None and dkl_row.shape[0] != M):
        raise _lib.AirHipError(f"gemm_grouped_gauss_bwd: pre {tuple(pre.shape)}, dpre {tuple(dpre.shape)}, eps {tuple(eps.shape)}")
    epi = _lib.AirGaussBwdEpi(int(problem), pre.data_ptr(), ld_pre, eps.data_ptr(), float(raw_offset), float(prior2[0]), float(prior2[1]),
                              loc.data_ptr(), scale.data_ptr(), dkl_row.data_ptr() if dkl_row is not None else None, float(dkl_scale),
                              dpre.data_ptr(), ld_dpre, D, float(guard_eps))
    dev = eps.device
    riders, nv, B = {}, (None, 0, None, None, None, None, None, None), 0
    ema = None
    if nvil is not None:
        parts = _f32(nvil["imp_parts"], "imp_parts", 2); base = _f32(nvil["baseline"], "baseline", 1); logp = _f32(nvil["logp"], "logp", 1)
        ema = _f32(nvil.get("ema"), "ema", 1)
        n_parts, B = parts.shape
        if base.shape[0] != B or logp.shape[0] != B or (ema is not None and ema.numel() != 4):
            raise _lib.AirHipError("gemm_grouped_gauss_bwd: baseline / logp hold B entries, ema four floats")
        riders = dict(out=_nan(4, device=dev), dlogp=_nan(B, device=dev), dbaseline=_nan(B, device=dev), imp_sum=_nan(B, device=dev))
        nv = (_p(parts), n_parts, _p(riders["imp_sum"]), _p(base), _p(logp), _p(riders["out"]), _p(riders["dlogp"]), _p(riders["dbaseline"]))
    klp, n_kl, kl_out = None, 0, None
    if kl_parts is not None:
        kl_parts = _f32(kl_parts, "kl_parts", 2)
        if kl_parts.shape[1] != M:
            raise _lib.AirHipError(f"gemm_grouped_gauss_bwd: kl_parts {tuple(kl_parts.shape)} for {M} rows")
        n_kl = kl_parts.shape[0]
        riders["kl_row"] = kl_out = _nan(M, device=dev)
        klp = kl_parts
    st = _status(lib().air_gemm_grouped_gauss_bwd(arr, len(outs), ctypes.byref(epi), *nv, B, _p(ema), _p(klp), n_kl, _p(kl_out), M,
                                                  _stream()), "air_gemm_grouped_gauss_bwd")
    return st, outs, riders


def gauss_sample_bwd_nvil(pre, eps, raw_offset, prior2, loc, scale, dsample, dkl_row, dkl_scale, dpre, guard_eps=0.0, nvil=None,
                          kl_parts=None):
    """air_gauss_sample_bwd_nvil (loc_mode 0, one prior; air_gauss_sample_bwd when nvil is None): the launch
    air_gemm_grouped_gauss_bwd folds away; arguments and riders as there, dsample[M, D] given"""
    ld_pre, ld_dpre = _mat(pre, "pre"), _mat(dpre, "dpre")
    eps = _f32(eps, "eps", 2); dsample = _f32(dsample, "dsample", 2); dkl_row = _f32(dkl_row, "dkl_row", 1)
    M, D = eps.shape
    dev = eps.device
    riders, nv, B, ema = {}, (None, 0, None, None, None, None, None, None), 0, None
    if nvil is not None:
        parts = _f32(nvil["imp_parts"], "imp_parts", 2); ema = _f32(nvil.get("ema"), "ema", 1)
        n_parts, B = parts.shape
        riders = dict(out=_nan(4, device=dev), dlogp=_nan(B, device=dev), dbaseline=_nan(B, device=dev), imp_sum=_nan(B, device=dev))
        nv = (_p(parts), n_parts, _p(riders["imp_sum"]), _p(_f32(nvil["baseline"], "baseline", 1)), _p(_f32(nvil["logp"], "logp", 1)),
              _p(riders["out"]), _p(riders["dlogp"]), _p(riders["dbaseline"]))
    n_kl, kl_out = 0, None
    if kl_parts is not None:
        n_kl = kl_parts.shape[0]
        riders["kl_row"] = kl_out = _nan(M, device=dev)
    pl, ps = float(prior2[0]), float(prior2[1])
    head = (_p(pre), ld_pre, _p(eps), float(raw_offset), 0, pl, ps, pl, ps, _p(_f32(loc, "loc", 2)), _p(_f32(scale, "scale", 2)),
            _p(dsample), None, _p(dkl_row), float(dkl_scale), _p(dpre), ld_dpre, M, D)
    kl = (_p(_f32(kl_parts, "kl_parts", 2)), n_kl, _p(kl_out))
    if nvil is None:                                                    # (that entry requires the NVIL rider)
        _lib.check(lib().air_gauss_sample_bwd(*head, float(guard_eps), *kl, _stream()), "air_gauss_sample_bwd")
    else:
        _lib.check(lib().air_gauss_sample_bwd_nvil(*head, *nv, B, float(guard_eps), _p(ema), *kl, _stream()), "air_gauss_sample_bwd_nvil")
    return riders


def batch_gather(dataset, seed_dev, step_dev, shuffle, B, out=None, want_idx=True):
    """air_batch_gather: dataset[n_items, item_floats] -> out[B, item_floats] (NaN-primed unless given), idx[B] int64 | None"""
    dataset = _f32(dataset, "dataset", 2)
    n_items, item_floats = dataset.shape
    if out is None:
        out = _nan(B, item_floats, device=dataset.device)
    idx = torch.full((B,), -1, dtype=torch.int64, device=dataset.device) if want_idx else None
    _lib.check(lib().air_batch_gather(_p(dataset), n_items, item_floats, _p(_i64(seed_dev, "seed_dev")), _p(_i64(step_dev, "step_dev")),
                                      int(bool(shuffle)), _p(out), int(B), _p(idx), _stream()), "air_batch_gather")
    return out, idx


def batch_gather_desc(dataset, seed_dev, step_dev, shuffle, obs, idx_out=None, copy_mask=0, n_items=None, item_floats=None):
    """AirBatchGather: rows of obs[B, item_floats] are drawn from dataset[n_items, item_floats] (the sizes may be overridden: what the
    launch is told, for the shapes it declines)"""
    return _lib.AirBatchGather(dataset.data_ptr(), int(dataset.shape[0] if n_items is None else n_items),
                               int(dataset.shape[1] if item_floats is None else item_floats), int(bool(shuffle)), int(obs.shape[0]),
                               _i64(seed_dev, "seed_dev").data_ptr(), _i64(step_dev, "step_dev").data_ptr(), obs.data_ptr(),
                               idx_out.data_ptr() if idx_out is not None else None, int(copy_mask))


def gemm_grouped_gather_fits(problems, bg, precision=0):
    """air_gemm_grouped_gather_fits: 1 when air_gemm_grouped_gather takes the group (every A a column window of bg's obs), else 0"""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped_gather_fits")
    return int(lib().air_gemm_grouped_gather_fits(arr, len(outs), ctypes.byref(bg)))


def gemm_grouped_gather(problems, bg, precision=0):
    """air_gemm_grouped_gather -> (status, [(C, colsum|None)]); status is 0 or AIR_E_UNSUPPORTED (nothing launched)"""
    arr, outs, keep = _gemm_descs(problems, precision, "gemm_grouped_gather")
    st = _status(lib().air_gemm_grouped_gather(arr, len(outs), ctypes.byref(bg), _stream()), "air_gemm_grouped_gather")
    return st, outs


def _prologue_tail(normal, uniform, rng_state_dev, global_step_dev, prior_out, T, init, final_value, anneal_type, anneal_steps, hold_for,
                   steps_div):
    """(normal, n_normal, uniform, n_uniform, rng_state, global_step, anneal_type, init, final, anneal_steps, hold_for, steps_div,
    prior_out, T): the argument run every entry point with the step prologue shares.  normal / uniform: flat float32 tensors | None."""
    if anneal_type not in ANNEAL_TYPES:
        raise _lib.AirHipError(f"step prologue: anneal_type must be one of {list(ANNEAL_TYPES)}")
    if prior_out.dtype != torch.float64 or not prior_out.is_cuda or prior_out.numel() < int(T) + 1:
        raise _lib.AirHipError("step prologue: prior_out must be a float64 CUDA tensor of T + 1 entries")
    normal = _f32(normal, "normal", 1); uniform = _f32(uniform, "uniform", 1)
    return (_p(normal), ctypes.c_size_t(normal.numel() if normal is not None else 0), _p(uniform),
            ctypes.c_size_t(uniform.numel() if uniform is not None else 0), _p(_i64(rng_state_dev, "rng_state_dev", 2)),
            _p(_i64(global_step_dev, "global_step_dev")), ANNEAL_TYPES[anneal_type], float(init), float(final_value), float(anneal_steps),
            float(hold_for), float(steps_div), _p(prior_out), int(T))


def step_prologue(normal, uniform, rng_state_dev, global_step_dev, T, h0, c0, B, init, final_value=0.0, anneal_type=None, anneal_steps=1.0,
                  hold_for=0.0, steps_div=1.0, x=None, gather=None):
    """air_step_prologue; with x[n] given air_step_prologue_cvt (-> the bf16 mirror of x); with gather = batch_gather_desc(...)
    air_step_prologue_gather_cvt (rows drawn from the dataset into the descriptor's obs and into the mirror).  normal / uniform: the flat
    buffers to fill (None: no draw).  -> prior[T+1] float64, h_tiled, c_tiled [B, Hd], x_bf16 | None; all NaN-primed"""
    h0 = _f32(h0, "h0"); c0 = _f32(c0, "c0")
    Hd = h0.numel()
    dev = h0.device
    prior = torch.full((int(T) + 1,), float("nan"), dtype=torch.float64, device=dev)
    h_t, c_t = _nan(B, Hd, device=dev), _nan(B, Hd, device=dev)
    args = _prologue_tail(normal, uniform, rng_state_dev, global_step_dev, prior, T, init, final_value, anneal_type, anneal_steps,
                          hold_for, steps_div) + (_p(h0), _p(c0), _p(h_t), _p(c_t), int(B), Hd)
    x16 = None
    if gather is not None:
        x16 = torch.full((gather.B, gather.item_floats), float("nan"), dtype=torch.bfloat16, device=dev)
        _lib.check(lib().air_step_prologue_gather_cvt(*args, ctypes.byref(gather), _p(x16), _stream()), "air_step_prologue_gather_cvt")
    elif x is not None:
        x = _f32(x, "x")
        x16 = torch.full(tuple(x.shape), float("nan"), dtype=torch.bfloat16, device=dev)
        _lib.check(lib().air_step_prologue_cvt(*args, _p(x), _p(x16), ctypes.c_size_t(x.numel()), _stream()), "air_step_prologue_cvt")
    else:
        _lib.check(lib().air_step_prologue(*args, _stream()), "air_step_prologue")
    return prior, h_t, c_t, x16


def lstm_step_fwd_prologue(h0, c0, w_h, gx, forget_bias, precision, normal, uniform, rng_state_dev, global_step_dev, T, init,
                           final_value=0.0, anneal_type=None, anneal_steps=1.0, hold_for=0.0, steps_div=1.0):
    """air_lstm_step_fwd_prologue: h0, c0 [Hd] (one row for the batch), w_h[Hd, 4Hd] and gx[M, 4Hd] (row views are fine)
    -> (h, c [M, Hd], gate_act[M, 4Hd]), (prior[T+1] float64, h_tiled, c_tiled [M, Hd]); all NaN-primed"""
    h0 = _f32(h0, "h0"); c0 = _f32(c0, "c0")
    Hd = h0.numel()
    ldw, ldgx = _mat(w_h, "w_h", 4 * Hd), _mat(gx, "gx", 4 * Hd)
    M = gx.shape[0]
    dev = gx.device
    h, c, act = _nan(M, Hd, device=dev), _nan(M, Hd, device=dev), _nan(M, 4 * Hd, device=dev)
    prior = torch.full((int(T) + 1,), float("nan"), dtype=torch.float64, device=dev)
    h_t, c_t = _nan(M, Hd, device=dev), _nan(M, Hd, device=dev)
    tail = _prologue_tail(normal, uniform, rng_state_dev, global_step_dev, prior, T, init, final_value, anneal_type, anneal_steps, hold_for,
                          steps_div)
    _lib.check(lib().air_lstm_step_fwd_prologue(_p(h0), _p(c0), _p(w_h), ldw, _p(gx), ldgx, _p(h), _p(c), _p(act), M, Hd, float(forget_bias),
                                                int(precision), *tail, _p(h_t), _p(c_t), _stream()), "air_lstm_step_fwd_prologue")
    return (h, c, act), (prior, h_t, c_t)


def lstm_first_step_fwd(x, w_x, b_gates, h0, c0, w_h, gx_out, forget_bias, precision, normal, uniform, rng_state_dev, global_step_dev, T,
                        init, final_value=0.0, anneal_type=None, anneal_steps=1.0, hold_for=0.0, steps_div=1.0):
    """air_lstm_first_step_fwd: x[M, E] (a row view is fine: ldx), w_x[E, 4Hd] and w_h[Hd, 4Hd] of ONE leading dimension, b_gates[4Hd],
    gx_out[M, 4Hd] (a row view of the caller's buffer: ldgx) -> status (0 | AIR_E_UNSUPPORTED), (h, c, gate_act), (prior, h_tiled, c_tiled)"""
    h0 = _f32(h0, "h0"); c0 = _f32(c0, "c0"); b_gates = _f32(b_gates, "b_gates", 1)
    Hd = h0.numel()
    ldx = _mat(x, "x")
    M, E = x.shape
    ldw, ldgx = _mat(w_h, "w_h", 4 * Hd), _mat(gx_out, "gx_out", 4 * Hd)
    if _mat(w_x, "w_x", 4 * Hd) != ldw or w_x.shape[0] != E or gx_out.shape[0] != M or b_gates.numel() != 4 * Hd:
        raise _lib.AirHipError(f"lstm_first_step_fwd: x {tuple(x.shape)}, w_x {tuple(w_x.shape)} (ld {w_x.stride(0)}), w_h ld {ldw}")
    dev = x.device
    h, c, act = _nan(M, Hd, device=dev), _nan(M, Hd, device=dev), _nan(M, 4 * Hd, device=dev)
    prior = torch.full((int(T) + 1,), float("nan"), dtype=torch.float64, device=dev)
    h_t, c_t = _nan(M, Hd, device=dev), _nan(M, Hd, device=dev)
    tail = _prologue_tail(normal, uniform, rng_state_dev, global_step_dev, prior, T, init, final_value, anneal_type, anneal_steps, hold_for,
                          steps_div)
    st = _status(lib().air_lstm_first_step_fwd(_p(x), ldx, E, _p(w_x), _p(b_gates), _p(h0), _p(c0), _p(w_h), ldw, _p(gx_out), ldgx, _p(h),
                                               _p(c), _p(act), M, Hd, float(forget_bias), int(precision), *tail, _p(h_t), _p(c_t),
                                               _stream()), "air_lstm_first_step_fwd")
    return st, (h, c, act), (prior, h_t, c_t)


def _canvas_bwd_args(glimpse, where, presence, obs, final_canvas):
    glimpse = _f32(glimpse, "glimpse", 4); where = _f32(where, "where", 3); presence = _f32(presence, "presence", 2)
    obs = _f32(obs, "obs", 3); final_canvas = _f32(final_canvas, "final_canvas", 3)
    T, B, h, w = glimpse.shape
    H, W = obs.shape[1:]
    if tuple(where.shape) != (T, B, 4) or tuple(presence.shape) != (T, B) or obs.shape[0] != B:
        raise _lib.AirHipError(f"canvas backward: glimpse {tuple(glimpse.shape)}, where {tuple(where.shape)}, presence {tuple(presence.shape)}")
    dg = _nan(T, B, h, w, device=glimpse.device); dwhere = _nan(T, B, 4, device=glimpse.device)
    return (_p(glimpse), _p(where), _p(presence), _p(obs), _p(final_canvas), _p(dg), _p(dwhere)), (T, B, H, W, h, w), dg, dwhere


def canvas_unroll_bwd_dpresence(glimpse, where, presence, obs, final_canvas, mult, std, loss_scale):
    """air_canvas_unroll_bwd_dpresence -> dglimpse[T,B,h,w], dwhere[T,B,4], dpresence[T,B] (NaN-primed)"""
    ptrs, dims, dg, dwhere = _canvas_bwd_args(glimpse, where, presence, obs, final_canvas)
    dpres = _nan(dims[0], dims[1], device=dg.device)
    _lib.check(lib().air_canvas_unroll_bwd_dpresence(*ptrs, _p(dpres), *dims, float(mult), float(std), float(loss_scale), _stream()),
               "air_canvas_unroll_bwd_dpresence")
    return dg, dwhere, dpres


def canvas_unroll_bwd_nvil(glimpse, where, presence, obs, final_canvas, mult, std, loss_scale, imp_parts, baseline, logp, ema=None):
    """air_canvas_unroll_bwd_nvil -> dglimpse, dwhere, (out[4], dlogp[B], dbaseline[B], imp_sum[B]) (NaN-primed)"""
    ptrs, dims, dg, dwhere = _canvas_bwd_args(glimpse, where, presence, obs, final_canvas)
    imp_parts = _f32(imp_parts, "imp_parts", 2); baseline = _f32(baseline, "baseline", 1); logp = _f32(logp, "logp", 1)
    ema = _f32(ema, "ema", 1)
    n_parts, B = imp_parts.shape
    if B != dims[1] or baseline.shape[0] != B or logp.shape[0] != B or (ema is not None and ema.numel() != 4):
        raise _lib.AirHipError("canvas_unroll_bwd_nvil: imp_parts[n_parts, B], baseline[B], logp[B], ema of four floats")
    dev = dg.device
    out, dlogp, dbase, imp_sum = _nan(4, device=dev), _nan(B, device=dev), _nan(B, device=dev), _nan(B, device=dev)
    _lib.check(lib().air_canvas_unroll_bwd_nvil(*ptrs, *dims, float(mult), float(std), float(loss_scale), _p(imp_parts), n_parts,
                                                _p(imp_sum), _p(baseline), _p(logp), _p(out), _p(dlogp), _p(dbase), _p(ema), _stream()),
               "air_canvas_unroll_bwd_nvil")
    return dg, dwhere, (out, dlogp, dbase, imp_sum)


def sum_leading(x):
    """air_sum_leading: x[T, n] -> out[n] = sum_t x[t], added in order from t = 0"""
    x = _f32(x, "x", 2)
    T, n = x.shape
    out = _nan(n, device=x.device)
    _lib.check(lib().air_sum_leading(_p(x), _p(out), T, ctypes.c_size_t(n), _stream()), "air_sum_leading")
    return out


def l2_grad_add_(g, p, ranges, l2_weight):
    """air_l2_grad_add: g += l2_weight * p on the (lo, hi) slices of the flat buffers, in place"""
    g = _f32(g, "g", 1); p = _f32(p, "p", 1)
    lo = (ctypes.c_size_t * len(ranges))(*[int(r[0]) for r in ranges]); hi = (ctypes.c_size_t * len(ranges))(*[int(r[1]) for r in ranges])
    if any(not (0 <= r[0] <= r[1] <= g.numel()) for r in ranges) or p.numel() != g.numel():
        raise _lib.AirHipError("l2_grad_add_: ranges must lie inside the flat buffers")
    _lib.check(lib().air_l2_grad_add(_p(g), _p(p), lo, hi, len(ranges), float(l2_weight), _stream()), "air_l2_grad_add")


def counter_add_(counter_dev, increment):
    """air_counter_add: counter_dev[0] += increment on the device"""
    _lib.check(lib().air_counter_add(_p(_i64(counter_dev, "counter_dev")), int(increment), _stream()), "air_counter_add")


# ---- tiled scene parsing -------------------------------------------------------------------------------------------
def tile_gather(scenes, img_size, stride):
    """air_tile_gather: scenes[S, Hs, Ws] -> windows[S * Nw, H * W] (bit copies; tile.py states the window order)"""
    from .tile import check_geometry
    scenes = _f32(scenes, "scenes", 3)
    S, Hs, Ws = scenes.shape
    (H, W) = img_size
    _, (sy, sx), (ny, nx) = check_geometry((Hs, Ws), (H, W), stride, n_scenes=S)
    out = _nan(S * ny * nx, H * W, device=scenes.device)
    _lib.check(lib().air_tile_gather(_p(scenes), S, Hs, Ws, H, W, sy, sx, _p(out), _stream()), "air_tile_gather")
    return out


def tile_merge(what, where, glimpse, score, num_objects, scene_size, img_size, stride, iou_merge=0.5):
    """air_tile_merge on a provider's rows what[T, R, A], where[T, R, 4], glimpse[T, R, G], score[T, R], num_objects[R] int32
    (R = S * Nw).  Returns a dict: what [C, S, A], where [C, S, 4], glimpse [C, S, G], score_src [C, S] (rows beyond a scene's count
    hold NaN: the entry does not write them), kept_cand [C, S], num_objects [S], cand_state [S, Nc] int8, dup_of [S, Nc],
    merge_counts [S, 6]."""
    from .tile import MAX_SLOTS, check_geometry
    what, where, glimpse, score = _f32(what, "what", 3), _f32(where, "where", 3), _f32(glimpse, "glimpse", 3), _f32(score, "score", 2)
    T, R, A = what.shape
    G = glimpse.shape[2]
    if where.shape != (T, R, 4) or glimpse.shape[:2] != (T, R) or score.shape != (T, R):
        raise _lib.AirHipError("tile_merge: where / glimpse / score do not match what[T, R, A]")
    if num_objects.dtype != torch.int32 or num_objects.shape != (R,) or not num_objects.is_cuda or not num_objects.is_contiguous():
        raise _lib.AirHipError("tile_merge: num_objects must be a contiguous int32 HIP tensor of R entries")
    (Hs, Ws), (H, W) = scene_size, img_size
    _, (sy, sx), (ny, nx) = check_geometry((Hs, Ws), (H, W), stride, T)
    Nw = ny * nx
    if R % Nw:
        raise _lib.AirHipError("tile_merge: %d rows are no multiple of %d windows" % (R, Nw))
    S, Nc, C = R // Nw, Nw * T, min(Nw * T, MAX_SLOTS)
    dev = what.device
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    out = {"what": _nan(C, S, A, device=dev), "where": _nan(C, S, 4, device=dev), "glimpse": _nan(C, S, G, device=dev),
           "score_src": _nan(C, S, device=dev), "kept_cand": i32(C, S), "num_objects": i32(S),
           "cand_state": torch.zeros((S, Nc), dtype=torch.int8, device=dev), "dup_of": i32(S, Nc), "merge_counts": i32(S, 6)}
    _lib.check(lib().air_tile_merge(_p(what), _p(where), _p(glimpse), _p(score), _p(num_objects), T, S, A, G, Hs, Ws, H, W, sy, sx,
                                    float(iou_merge), _p(out["what"]), _p(out["where"]), _p(out["glimpse"]), _p(out["score_src"]),
                                    _p(out["kept_cand"]), _p(out["num_objects"]), _p(out["cand_state"]), _p(out["dup_of"]),
                                    _p(out["merge_counts"]), _stream()), "air_tile_merge")
    return out
