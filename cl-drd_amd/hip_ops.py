"""Typed Python wrappers over the C ABI (include/cldrd_hip.h): torch tensors in, device pointers out.

PyTorch is only plumbing here (device memory + the current HIP stream); every wrapper checks dtype / layout /
device on the host (the reference raises Python exceptions before launch) and then calls
the kernel.  There is no fallback: tensors must live on a GPU.
"""
from __future__ import annotations

import torch

import os
import threading

from . import _lib
from ._lib import call

BF16 = torch.bfloat16
F32 = torch.float32
F16 = torch.float16


FMT_BF16, FMT_F16, FMT_F16_C_BF16, FMT_F16_TAPE = 0, 1, 3, 5        # enum cldrd_fmt16 of include/cldrd_hip.h (tests/test_capi.py compares)

_SPLITK_WS = {}       # (M, N, K, gemm_splitk, gemm_nt64) -> cldrd_gemm_nt_splitk_workspace(M, N, K): everything the library's launch plan reads
_TUNING = {}          # what set_tuning() has set


def _fmt16(t, name):
    """16-bit activation format of a forward operand: bf16 (default) or fp16 (high-precision forward of the query tower)."""
    if t.dtype not in (BF16, F16):
        raise TypeError(f"{name}: expected bf16 or fp16, got {t.dtype}")
    return FMT_F16 if t.dtype == F16 else FMT_BF16


def _gemm_fmt(A, out, preact, gelu_pre):
    """The format code of one gemm_nt call: fp16 operands give an fp16 C, or a bf16 C where ``out`` is one (the QKV projection in front of
    the bf16 attention kernels); an fp16 tape (``preact`` / ``gelu_pre``: the all-fp16 training mode) makes it FMT_F16_TAPE."""
    fmt = _fmt16(A, "A")
    if fmt == FMT_F16 and out.dtype == BF16:
        fmt = FMT_F16_C_BF16
    for t, n in ((preact, "preact"), (gelu_pre, "gelu_pre")):
        if t is not None and t.dtype == F16:          # the all-fp16 training mode: gelu'(x) lives on the tape in fp16 too
            if fmt not in (FMT_F16, FMT_F16_TAPE):
                raise TypeError(f"gemm_nt: an fp16 {n} goes with fp16 operands and an fp16 / fp32 out")
            fmt = FMT_F16_TAPE
    return fmt


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Raw handle of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream object per call
    (~5 us: device index resolution, availability check) - a fifth of the host time of a training step at ~230 calls per step."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, dtype, name, dim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must be on the GPU (cldrd_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"{name}: expected {dim} dims, got {t.dim()}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dim must be contiguous")
    return t


_TLS = threading.local()      # the library keeps these pointers per thread: so does the mirror that lets the contexts nest


class seed_base:
    """``with seed_base(ptr):`` every launch inside passes its ``seed`` argument as an OFFSET: the kernels add the 64-bit word at the device
    address ``ptr`` at run time (include/cldrd_hip.h: cldrd_set_seed_base).  ``ptr`` None / 0: a no-op context."""

    def __init__(self, ptr):
        self.ptr = int(ptr) if ptr else None

    def __enter__(self):
        if self.ptr:
            self.prev = getattr(_TLS, "seed_base", None)        # contexts nest (two towers): restore, do not clear
            _lib.load().cldrd_set_seed_base(self.ptr)
            _TLS.seed_base = self.ptr

    def __exit__(self, *exc):
        if self.ptr:
            _lib.load().cldrd_set_seed_base(self.prev)
            _TLS.seed_base = self.prev


class loss_scale:
    """``with loss_scale(ptr, interval):`` launches inside apply the loss scale at device address ``ptr`` (the float[72] block of
    ``new_loss_scale_state``; include/cldrd_hip.h: cldrd_set_loss_scale).  ``ptr`` None / 0: a no-op context."""

    def __init__(self, ptr, interval=2000):
        self.ptr, self.interval = (int(ptr) if ptr else None), int(interval)

    def __enter__(self):
        if self.ptr:
            self.prev = getattr(_TLS, "loss_scale", None)
            _lib.load().cldrd_set_loss_scale(self.ptr, self.interval)
            _TLS.loss_scale = (self.ptr, self.interval)

    def __exit__(self, *exc):
        if self.ptr:
            prev = self.prev or (None, 0)
            _lib.load().cldrd_set_loss_scale(prev[0], prev[1])
            _TLS.loss_scale = self.prev


class norm_sink:
    """``with norm_sink(slots) as sink:`` weight-gradient slab reductions and LayerNorm-parameter reductions launched inside also write
    per-workgroup sums of squares of the gradients they write to ``slots`` (fp32, device); ``sink.used`` afterwards = slots written, or -1
    when a launch inside could not contribute (include/cldrd_hip.h: cldrd_set_norm_sink).  ``slots`` None: a no-op context (used = -1)."""

    def __init__(self, slots):
        self.slots, self.used = slots, -1

    def __enter__(self):
        if self.slots is not None:
            _chk(self.slots, F32, "slots", 1)
            _lib.load().cldrd_set_norm_sink(self.slots.data_ptr(), self.slots.numel())
        return self

    def __exit__(self, *exc):
        if self.slots is not None:
            lib = _lib.load()
            self.used = int(lib.cldrd_norm_sink_used())
            lib.cldrd_set_norm_sink(None, 0)


def new_loss_scale_state(device):
    """device float[72]: {S = 1, 1 / S = 1, good steps 0, skipped 0, headroom exponent 0, ..., scratch} (include/cldrd_hip.h)"""
    st = torch.zeros(72, dtype=F32, device=device)
    st[0] = 1.0
    st[1] = 1.0
    return st


def loss_scale_adapt(a, b, state):
    """S from max(|a|, |b|) (fp32 tensors: dL/dCLS of the two towers), written to ``state``; a and b are multiplied by S in place."""
    _chk(state, F32, "state", 1)
    if state.numel() < 72:
        raise ValueError("loss_scale_adapt: state is a float[72] from new_loss_scale_state()")
    for t, n in ((a, "a"), (b, "b")):
        if t is not None:
            _chk(t, F32, n)
            if not t.is_contiguous():
                raise ValueError("loss_scale_adapt: contiguous tensors")
    call("cldrd_loss_scale_adapt", _p(a), a.numel() if a is not None else 0, _p(b), b.numel() if b is not None else 0, _p(state), _stream())


class optim_hyper:
    """``with optim_hyper(ptr):`` adamw_step launches inside read {lr, step size} from the device float[2] at ``ptr``."""

    def __init__(self, ptr):
        self.ptr = int(ptr) if ptr else None

    def __enter__(self):
        if self.ptr:
            self.prev = getattr(_TLS, "optim_hyper", None)
            _lib.load().cldrd_set_optim_hyper(self.ptr)
            _TLS.optim_hyper = self.ptr

    def __exit__(self, *exc):
        if self.ptr:
            _lib.load().cldrd_set_optim_hyper(self.prev)
            _TLS.optim_hyper = self.prev


def write_step_state(seeds, seed0, seed1, hyper, lr, beta1, beta2, adam_step, scale_state=None):
    """seeds: device int64[>= 2]; hyper: device float32[>= 2] (either may be None).  ``scale_state`` (the float[72] loss-scale block,
    optional): Adam's bias-correction exponent becomes ``adam_step`` minus the steps the safety net skipped, read on the device."""
    if scale_state is not None:
        _chk(scale_state, F32, "scale_state", 1)
        if scale_state.numel() < 72:
            raise ValueError("write_step_state: scale_state is the float[72] block of new_loss_scale_state()")
    call("cldrd_write_step_state", _p(seeds), int(seed0) & 0xFFFFFFFFFFFFFFFF, int(seed1) & 0xFFFFFFFFFFFFFFFF, _p(hyper), float(lr), float(beta1),
         float(beta2), int(adam_step), _p(scale_state), _stream())


def copy_segments(dsts, srcs):
    """dst[i] <- src[i] for up to 8 pairs of same-sized contiguous device tensors in one launch (bytes are copied: same dtype expected)."""
    import ctypes as C
    n = len(dsts)
    if n != len(srcs) or not 1 <= n <= 8:
        raise ValueError("copy_segments: 1..8 (dst, src) pairs")
    for d, s_ in zip(dsts, srcs):
        if not (d.is_cuda and s_.is_cuda and d.is_contiguous() and s_.is_contiguous() and d.dtype == s_.dtype and d.numel() == s_.numel()):
            raise ValueError("copy_segments: contiguous device tensors of equal dtype and size")
    src = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dst = (C.c_void_p * n)(*[t.data_ptr() for t in dsts])
    nb = (C.c_size_t * n)(*[t.numel() * t.element_size() for t in srcs])
    call("cldrd_copy_segments", src, dst, nb, n, _stream())


def zero_segments(tensors):
    """up to 8 contiguous device tensors (16-byte aligned, byte sizes multiples of 16) set to zero in one launch (cldrd_zero_segments)"""
    import ctypes as C
    n = len(tensors)
    if not 1 <= n <= 8:
        raise ValueError("zero_segments: 1..8 tensors")
    for t in tensors:
        _chk(t, t.dtype, "zero_segments")
        if not t.is_contiguous():
            raise ValueError("zero_segments: contiguous tensors")
    dst = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    nb = (C.c_size_t * n)(*[t.numel() * t.element_size() for t in tensors])
    call("cldrd_zero_segments", dst, nb, n, _stream())


def pad_rows(rows: int) -> int:
    """Activation / gradient buffers are allocated with rows rounded up to 64 (allocation granularity only: no kernel reads the
    rows past M any more - the weight-gradient kernel fetches them from a zero page)."""
    return (rows + 63) // 64 * 64


def gemm_nt(A, B, out, M=None, *, bias=None, residual=None, preact=None, gelu_pre=None, act=0, alpha=1.0,
            dropout_p=0.0, seed=0, residual_ln=None):
    """out[M,N] = epilogue(alpha * A[M,K] @ B[N,K]^T); A, B bf16 (or both fp16: forward flavours, M < 1024); out 16-bit like A, or fp32.

    A, B, out and residual take row pitches (``stride(0)``); ``preact`` / ``gelu_pre`` are [>= M, N] views with the row pitch of ``out``.
    ``act``: bit 0 = erf-GELU; bit 1 = derivative form: ``preact`` receives gelu'(pre-activation) (act=3), ``gelu_pre`` holds it (act=2).
    ``residual_ln`` = (mean[M], rstd[M], gamma[N], beta[N]): the fp32 ``residual`` is a pre-LN sum and LayerNorm(residual) is what is added.
    fp16 operands with M >= 1024: the forward FFN flavours only (bias + GELU [+ tape]; bias [+ dropout] + residual_ln -> fp32 out)."""
    fmt = _gemm_fmt(A, out, preact, gelu_pre)
    _chk(A, A.dtype, "A", 2), _chk(B, A.dtype, "B", 2)
    M = A.shape[0] if M is None else M
    N, K = B.shape
    if A.shape[1] != K or out.shape[1] != N or out.shape[0] < M or A.shape[0] < M:
        raise ValueError(f"gemm_nt: shape mismatch A{tuple(A.shape)} B{tuple(B.shape)} out{tuple(out.shape)} M={M}")
    out_f32 = 1 if out.dtype == F32 else 0
    if not out_f32:
        _chk(out, F16 if fmt in (FMT_F16, FMT_F16_TAPE) else BF16, "out", 2)
    if bias is not None:
        _chk(bias, F32, "bias", 1)
        if bias.numel() != N:
            raise ValueError("gemm_nt: bias must be [N]")
    for t, n in ((preact, "preact"), (gelu_pre, "gelu_pre")):
        if t is not None:
            _chk(t, F16 if fmt == FMT_F16_TAPE else BF16, n, 2)
            # the tape has no leading dimension of its own in the C ABI: the kernels index it with out's
            if t.shape[0] < M or t.shape[1] != N or t.stride(0) != out.stride(0):
                raise ValueError(f"gemm_nt: {n} must be [>= M, N] with the row pitch of out")
    res_f32 = 0
    if residual is not None:
        res_f32 = 1 if residual.dtype == F32 else 0        # fp32: the residual stream kept in full precision
        _chk(residual, F32 if res_f32 else BF16, "residual", 2)
        if residual.shape[0] < M or residual.shape[1] != N:
            raise ValueError("gemm_nt: residual must be [>= M, N]")
    mean = rstd = gamma = beta = None
    if residual_ln is not None:
        mean, rstd, gamma, beta = residual_ln
        if not res_f32:
            raise ValueError("gemm_nt: residual_ln needs an fp32 residual (the pre-LN sum)")
        _chk(mean, F32, "ln mean", 1), _chk(rstd, F32, "ln rstd", 1), _chk(gamma, F32, "ln gamma", 1), _chk(beta, F32, "ln beta", 1)
        if mean.numel() < M or rstd.numel() < M or gamma.numel() != N or beta.numel() != N:
            raise ValueError("gemm_nt: residual_ln = (mean[>= M], rstd[>= M], gamma[N], beta[N])")
    # small-M problems (CLS-only last layer, query tower) are split along K when that fills the chip: fp32 partials in a scratch tensor
    ws, ws_bytes = None, 0
    if M < 1024:
        key = (M, N, K, _TUNING.get("gemm_splitk", 0), _TUNING.get("gemm_nt64", 1))
        ws_bytes = _SPLITK_WS.get(key)
        if ws_bytes is None:
            ws_bytes = _SPLITK_WS[key] = int(_lib.load().cldrd_gemm_nt_splitk_workspace(M, N, K))
        if ws_bytes:
            ws = torch.empty(ws_bytes // 4, dtype=F32, device=A.device)
    call("cldrd_gemm_nt16", _p(A), _p(B), _p(out), M, N, K, A.stride(0), B.stride(0), out.stride(0), _p(bias),
         _p(residual), residual.stride(0) if residual is not None else 0, _p(preact), _p(gelu_pre), act, alpha, dropout_p, seed,
         out_f32, res_f32, fmt, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(ws), ws_bytes, _stream())
    return out


def gemm_nt_f32(A, W, out, M=None, *, bias=None, residual=None, act=0):
    """out[M,N] = A[M,K] @ W[N,K]^T (+ bias) (act = 1: erf-GELU) (+ residual), every operand fp32, on the f32-input MFMA (the fp32 evaluation
    pass, csrc/encoder_f32.hip).  A, out and residual take row pitches (``stride(0)``): the CLS rows of a padded batch are a strided view.
    One schedule for every M: a row's result does not depend on the other rows of the launch."""
    _chk(A, F32, "A", 2), _chk(W, F32, "W", 2), _chk(out, F32, "out", 2)
    M = A.shape[0] if M is None else M
    N, K = W.shape
    if A.shape[1] != K or out.shape[1] != N or out.shape[0] < M or A.shape[0] < M or M < 1:
        raise ValueError(f"gemm_nt_f32: shape mismatch A{tuple(A.shape)} W{tuple(W.shape)} out{tuple(out.shape)} M={M}")
    if K % 32 or N % 8:
        raise ValueError("gemm_nt_f32: K must be a multiple of 32, N of 8")
    if bias is not None:
        _chk(bias, F32, "bias", 1)
        if bias.numel() != N:
            raise ValueError("gemm_nt_f32: bias must be [N]")
    if residual is not None:
        _chk(residual, F32, "residual", 2)
        if residual.shape[0] < M or residual.shape[1] != N:
            raise ValueError("gemm_nt_f32: residual must be [>= M, N]")
    if act not in (0, 1):
        raise ValueError("gemm_nt_f32: act is 0 or 1 (erf-GELU)")
    call("cldrd_gemm_nt_f32", _p(A), _p(W), _p(out), M, N, K, A.stride(0), W.stride(0), out.stride(0), _p(bias), _p(residual),
         residual.stride(0) if residual is not None else 0, act, _stream())
    return out


def set_tuning(key: str, value: int) -> None:
    """cldrd_set_tuning: "gemm_splitk" | "gemm_nt64" | "attn_fwd2" | "attn_bwd2" (include/cldrd_hip.h).  Process-wide; tests use it to reach the
    alternative kernels - the library itself reads no environment variable."""
    call("cldrd_set_tuning", key.encode(), int(value))
    _TUNING[key] = int(value)


def wgrad_workspace_elems(M, N1, N2) -> int:
    return _lib.load().cldrd_wgrad_splits(M, N1, N2) * (N1 * N2 + N1)


def wgrad(dY, X, dW, M, workspace, accumulate=False, dbias=None):
    """dW[N1,N2] (+)= dY[:M]^T @ X[:M] (and dbias[N1] (+)= column sums of dY[:M]); dY, X bf16 with >= M rows; dW, dbias fp32."""
    f16 = dY.dtype == F16
    _chk(dY, F16 if f16 else BF16, "dY", 2), _chk(X, F16 if f16 else BF16, "X", 2), _chk(dW, F32, "dW", 2), _chk(workspace, F32, "workspace")
    N1, N2 = dW.shape
    if dY.shape[1] != N1 or X.shape[1] != N2 or not dW.is_contiguous():
        raise ValueError("wgrad: shape mismatch")
    if dY.shape[0] < M or X.shape[0] < M:
        raise ValueError("wgrad: operands have fewer than M rows")
    if dbias is not None:
        _chk(dbias, F32, "dbias", 1)
    call("cldrd_wgrad16", _p(dY), _p(X), _p(dW), _p(dbias), M, N1, N2, dY.stride(0), X.stride(0), _p(workspace),
         workspace.numel() * 4, (1 if accumulate else 0) | (2 if f16 else 0), _stream())
    return dW


class WgradQueue:
    """Deferred weight gradients of one tower: ``add`` records a problem (and keeps its operands alive), ``flush`` hands everything
    recorded so far to ONE ``cldrd_wgrad_group`` launch on the current stream (include/cldrd_hip.h).  Only the data gradients are
    on the critical path of the backward; grouping the weight gradients removes the token splits, the fp32 slabs and ~50 launches
    per tower and step."""

    def __init__(self):
        self.jobs = []

    def add(self, dY, X, dW, M, dbias=None):
        f16 = dY.dtype == F16        # fp16 operands (the all-fp16 training mode); one format per queue
        _chk(dY, F16 if f16 else BF16, "dY", 2), _chk(X, F16 if f16 else BF16, "X", 2), _chk(dW, F32, "dW", 2)
        if self.jobs and (self.jobs[0][0].dtype == F16) != f16:
            raise TypeError("WgradQueue: fp16 and bf16 problems cannot share a launch")
        N1, N2 = dW.shape
        if dY.shape[1] != N1 or X.shape[1] != N2 or not dW.is_contiguous() or dY.shape[0] < M or X.shape[0] < M:
            raise ValueError("wgrad: shape mismatch")
        if dbias is not None:
            _chk(dbias, F32, "dbias", 1)
        self.jobs.append((dY, X, dW, dbias, int(M)))

    def __len__(self):
        return len(self.jobs)

    def flush(self, accumulate=False):
        jobs, self.jobs = self.jobs, []
        if not jobs:
            return
        import ctypes as C
        n = len(jobs)
        VP, IN = C.c_void_p * n, C.c_int * n
        A, B = VP(*[j[0].data_ptr() for j in jobs]), VP(*[j[1].data_ptr() for j in jobs])
        W, Bi = VP(*[j[2].data_ptr() for j in jobs]), VP(*[(j[3].data_ptr() if j[3] is not None else None) for j in jobs])
        Ms, N1s, N2s = IN(*[j[4] for j in jobs]), IN(*[j[2].shape[0] for j in jobs]), IN(*[j[2].shape[1] for j in jobs])
        lda, ldb = IN(*[j[0].stride(0) for j in jobs]), IN(*[j[1].stride(0) for j in jobs])
        need = _lib.load().cldrd_wgrad_group_workspace(Ms, N1s, N2s, n)
        ws = torch.empty(need, dtype=F32, device=jobs[0][2].device) if need else None
        call("cldrd_wgrad_group", A, B, W, Bi, Ms, N1s, N2s, lda, ldb, n, _p(ws), need * 4,
             (1 if accumulate else 0) | (2 if jobs[0][0].dtype == F16 else 0), _stream())
        # `jobs` held the operands alive until here; they were allocated on the stream this launch is on, so releasing them now
        # is ordered behind it by the caching allocator


def attention_drop_bits(nseq, L, H, dropout_p, device):
    """int32 buffer for the dropout keep bits the forward leaves for the backward at this shape, or None (the backward re-hashes)."""
    n = _lib.load().cldrd_attention_bits_words(nseq, L, H, dropout_p)
    return torch.empty(n, dtype=torch.int32, device=device) if n > 0 else None


def _cu_rows(cu, nseq, mask, what):
    """``cu`` (int32 [nseq + 1] on the device): the PACKED layout - sequence m owns rows cu[m] .. cu[m + 1] of every [Tp, .] tensor, keys beyond
    its length are masked (no mask tensor is read)."""
    _chk(cu, torch.int32, "cu", 1)
    if cu.numel() != nseq + 1 or not cu.is_contiguous():
        raise ValueError(f"{what}: cu must be contiguous int32 [nseq + 1]")
    if mask is not None:
        raise ValueError(f"{what}: a packed batch takes its key mask from cu (pass mask=None)")
    return cu


def _seq_list(seq_list, tile, cu, nseq, L, what):
    """``seq_list`` (int32 on the device) with ``tile``: the launch covers only these sequences of a packed batch, each at most ``tile`` <= L tokens
    long, with the kernels of that tile height."""
    if cu is None:
        raise ValueError(f"{what}: a sequence list goes with a packed batch (cu)")
    _chk(seq_list, torch.int32, "seq_list", 1)
    if not seq_list.is_contiguous() or not (0 < seq_list.numel() <= nseq) or not (0 < int(tile) <= L):
        raise ValueError(f"{what}: seq_list must be contiguous int32 with 1 .. nseq entries, 0 < tile <= L")
    return (_p(seq_list), int(seq_list.numel()), int(tile))


def _layout(mask, cu, seq_list, tile, nseq, L, what):
    """The (mask, cu_rows, seq_list, n_list, Ltile) arguments of an attention entry point (layout rule: include/cldrd_hip.h)."""
    lst = _seq_list(seq_list, tile, cu, nseq, L, what) if seq_list is not None else (None, 0, 0)
    if cu is not None:
        return (None, _p(_cu_rows(cu, nseq, mask, what)), *lst)
    return (_p(mask), None, *lst)


def _head_dim(head_dim, what, H=None, **training_only):
    """The ``head_dim`` keyword of the attention calls: 64 (every pass), or 32 - the evaluation forward of csrc/attention_hd32.hip, which has no
    dropout, tape or keep bits (``training_only``: the arguments that must then be unset) and, in the 16-bit kernels, needs an even ``H``."""
    if head_dim == 64:
        return 64
    if head_dim != 32:
        raise ValueError(f"{what}: head dim {head_dim} is not supported (the attention kernels exist for head dim 64 and 32)")
    bad = [k for k, v in training_only.items() if v]
    if bad:
        raise ValueError(f"{what}: head dim 32 runs the evaluation forward only: no {' / '.join(bad)}")
    if H is not None and H % 2:
        raise ValueError(f"{what}: head dim 32 needs an even number of heads, got {H}")
    return 32


def _attention_fwd_hd32(qkv, mask, ctx, nseq, L, H, ctx16, cu, seq_list, tile):
    what = "attention_fwd(head_dim=32)"
    fmt = _fmt16(qkv, "qkv")
    layout = _layout(mask, cu, seq_list, tile, nseq, L, what)
    dt16 = F16 if fmt else BF16
    _chk(qkv, dt16, "qkv", 2)
    if ctx is None and ctx16 is None:
        raise ValueError(f"{what}: no output")
    if ctx16 is not None and fmt:
        raise ValueError(f"{what}: ctx16 goes with a bf16 pass")
    for t, n, dt in ((ctx, "ctx", dt16), (ctx16, "ctx16", F16)):
        if t is not None:
            _chk(t, dt, n, 2)
            if t.shape[1] != H * 32 or not t.is_contiguous():
                raise ValueError(f"{what}: {n} must be contiguous [T, H*32]")
    if mask is not None:
        _chk(mask, torch.int64, "mask", 2)
        if not mask.is_contiguous() or tuple(mask.shape) != (nseq, L):
            raise ValueError(f"{what}: mask must be contiguous int64 [nseq, L]")
    if qkv.shape[1] != 3 * H * 32 or not qkv.is_contiguous():
        raise ValueError(f"{what}: qkv must be contiguous [T, 3*H*32]")
    call("cldrd_attention_fwd_hd32", _p(qkv), *layout, _p(ctx), nseq, L, H, fmt, _p(ctx16), _stream())
    return ctx16 if ctx is None else ctx


def attention_fwd(qkv, mask, ctx, lse, nseq, L, H, dropout_p=0.0, seed=0, drop_bits=None, ctx16=None, full_family=False, cu=None, seq_list=None, tile=0,
                  head_dim=64):
    """``ctx16`` (fp16, bf16 pass only): the same context in fp16, for an fp16-operand out-projection; ``ctx`` may then be None.
    ``cu``: qkv / ctx / ctx16 are packed [Tp, .] (see _cu_rows); ``lse`` and ``drop_bits`` keep their padded shapes.  ``seq_list`` / ``tile``:
    see _seq_list.  ``head_dim=32``: the evaluation forward at head dim 32 (shapes against H*32; bf16 or fp16 at every L <= 256; see _head_dim)."""
    if _head_dim(head_dim, "attention_fwd", H, dropout_p=dropout_p > 0, lse=lse is not None, drop_bits=drop_bits is not None, full_family=full_family) == 32:
        return _attention_fwd_hd32(qkv, mask, ctx, nseq, L, H, ctx16, cu, seq_list, tile)
    fmt = _fmt16(qkv, "qkv")
    layout = _layout(mask, cu, seq_list, tile, nseq, L, "attention_fwd")
    _chk(qkv, F16 if fmt else BF16, "qkv", 2)
    if ctx16 is not None:
        if fmt:
            raise ValueError("attention_fwd: ctx16 goes with a bf16 pass")
        _chk(ctx16, F16, "ctx16", 2)
        if ctx16.shape[1] != H * 64 or not ctx16.is_contiguous():
            raise ValueError("attention: ctx16 must be contiguous [T, H*64]")
    if ctx is not None or ctx16 is None:
        _chk(ctx, F16 if fmt else BF16, "ctx", 2)
    if mask is not None:
        _chk(mask, torch.int64, "mask", 2)
        if not mask.is_contiguous() or tuple(mask.shape) != (nseq, L):
            raise ValueError("attention: mask must be contiguous int64 [nseq, L]")
    if qkv.shape[1] != 3 * H * 64 or not qkv.is_contiguous() or (ctx is not None and (ctx.shape[1] != H * 64 or not ctx.is_contiguous())):
        raise ValueError("attention: qkv must be [T, 3*H*64], ctx [T, H*64], contiguous")
    if lse is not None:
        _chk(lse, F32, "lse")
    if drop_bits is not None:
        _chk(drop_bits, torch.int32, "drop_bits", 1)
        if drop_bits.numel() != _lib.load().cldrd_attention_bits_words(nseq, L, H, dropout_p):
            raise ValueError("attention_fwd: drop_bits must come from attention_drop_bits() for the same shape")
    if fmt == FMT_F16 and (drop_bits is not None or L > 128 or full_family):
        fmt = FMT_F16_TAPE            # fp16 through the whole kernel family of the bf16 path (persistent kernel, keep bits, L > 128)
    call("cldrd_attention_fwd", _p(qkv), *layout, _p(ctx), _p(lse), nseq, L, H, dropout_p, seed, fmt, _p(drop_bits), _p(ctx16), _stream())
    return ctx16 if ctx is None else ctx


def attention_bwd(qkv, mask, ctx, dctx, lse, dqkv, nseq, L, H, dropout_p=0.0, seed=0, drop_bits=None, cu=None, seq_list=None, tile=0):
    """``cu``: qkv / ctx / dctx / dqkv are packed [Tp, .] (see _cu_rows); ``seq_list`` / ``tile``: see _seq_list."""
    fmt = _fmt16(qkv, "qkv")       # fp16 everywhere (the all-fp16 training mode) or bf16 everywhere
    for t, n in ((qkv, "qkv"), (ctx, "ctx"), (dctx, "dctx"), (dqkv, "dqkv")):
        _chk(t, F16 if fmt else BF16, n, 2)
        if not t.is_contiguous():
            raise ValueError(f"attention_bwd: {n} must be contiguous")
    _chk(lse, F32, "lse")
    if drop_bits is not None:
        _chk(drop_bits, torch.int32, "drop_bits", 1)
    call("cldrd_attention_bwd", _p(qkv), *_layout(mask, cu, seq_list, tile, nseq, L, "attention_bwd"), _p(ctx), _p(dctx), _p(lse), _p(dqkv),
         nseq, L, H, dropout_p, seed, fmt, _p(drop_bits), _stream())
    return dqkv


def attention_cls_fwd(qc, kv, mask, ctx, probs, nseq, L, H, dropout_p=0.0, seed=0, ctx16=None, cu=None, head_dim=64):
    """``cu``: kv is packed [Tp, 2*H*64] (see _cu_rows); probs stays [nseq, H, L].  ``head_dim=32``: the evaluation form at head dim 32
    (kv [T, 2*H*32]; ``probs`` must be None: see _head_dim)."""
    hd = _head_dim(head_dim, "attention_cls_fwd", H, dropout_p=dropout_p > 0, probs=probs is not None)
    fmt = _fmt16(qc, "qc")
    dt16 = F16 if fmt else BF16
    if hd == 32:
        what = "attention_cls_fwd(head_dim=32)"
        _chk(qc, dt16, "qc", 2), _chk(kv, dt16, "kv", 2)
        if ctx is None and ctx16 is None:
            raise ValueError(f"{what}: no output")
        if ctx16 is not None and fmt:
            raise ValueError(f"{what}: ctx16 goes with a bf16 pass")
        for t, n, dt in ((ctx, "ctx", dt16), (ctx16, "ctx16", F16)):
            if t is not None:
                _chk(t, dt, n, 2)
                if t.shape[1] != H * 32 or t.shape[0] < nseq or not t.is_contiguous():
                    raise ValueError(f"{what}: {n} must be contiguous [nseq, H*32]")
        if kv.shape[1] != 2 * H * 32 or not kv.is_contiguous() or qc.shape[1] != H * 32 or qc.shape[0] < nseq or not qc.is_contiguous():
            raise ValueError(f"{what}: kv must be contiguous [T, 2*H*32], qc contiguous [nseq, H*32]")
        if mask is not None:
            _chk(mask, torch.int64, "mask", 2)
            if not mask.is_contiguous() or tuple(mask.shape) != (nseq, L):
                raise ValueError(f"{what}: mask must be contiguous int64 [nseq, L]")
        call("cldrd_attention_cls_fwd_hd32", _p(qc), _p(kv), *_layout(mask, cu, None, 0, nseq, L, what)[:2], _p(ctx), nseq, L, H, fmt, _p(ctx16),
             _stream())
        return
    _chk(qc, dt16, "qc", 2), _chk(kv, dt16, "kv", 2), _chk(probs, F32, "probs")
    if ctx is not None:
        _chk(ctx, dt16, "ctx", 2)
    if ctx16 is not None:
        if fmt:
            raise ValueError("attention_cls_fwd: ctx16 goes with a bf16 pass")
        _chk(ctx16, F16, "ctx16", 2)
    if ctx is None and ctx16 is None:
        raise ValueError("attention_cls_fwd: no output")
    if kv.shape[1] != 2 * H * 64 or not kv.is_contiguous() or not qc.is_contiguous() or any(t is not None and not t.is_contiguous() for t in (ctx, ctx16)):
        raise ValueError("attention_cls: kv must be contiguous [T, 2*H*64]")
    call("cldrd_attention_cls_fwd", _p(qc), _p(kv), *_layout(mask, cu, None, 0, nseq, L, "attention_cls_fwd")[:2], _p(ctx), _p(probs), nseq, L, H,
         dropout_p, seed, fmt, _p(ctx16), _stream())


def attention_cls_bwd(qc, kv, probs, dctx, dqc, dkv, nseq, L, H, dropout_p=0.0, seed=0, cu=None):
    """``cu``: kv and dkv are packed [Tp, 2*H*64] (see _cu_rows)."""
    fmt = _fmt16(qc, "qc")
    for t, n in ((qc, "qc"), (kv, "kv"), (dctx, "dctx"), (dqc, "dqc"), (dkv, "dkv")):
        _chk(t, F16 if fmt else BF16, n, 2)
        if not t.is_contiguous():
            raise ValueError(f"attention_cls_bwd: {n} must be contiguous")
    call("cldrd_attention_cls_bwd", _p(qc), _p(kv), _layout(None, cu, None, 0, nseq, L, "attention_cls_bwd")[1], _p(probs), _p(dctx), _p(dqc), _p(dkv),
         nseq, L, H, dropout_p, seed, fmt, _stream())


def attention_fwd_f32(qkv, mask, ctx, nseq, L, H, cu=None, qc=None, head_dim=64):
    """fp32 attention of the fp32 evaluation pass (csrc/encoder_f32.hip): ``ctx = softmax(Q K^T / 8 + key mask) V``, head dim 64, L <= 256.
    Full form (``qc`` None): ``qkv`` fp32 [T, 3*H*64], ``ctx`` [T, H*64].  CLS form (``qc`` fp32 [nseq, H*64], a row pitch allowed): ``qkv`` is
    K | V of every token, [T, 2*H*64], ``ctx`` [nseq, H*64] - bit for bit row 0 of the full form.  Layout: padded rows with ``mask`` (int64
    [nseq, L] or None) or packed rows through ``cu`` (see _cu_rows), never both.  ``head_dim=32``: the same at head dim 32 (every 64 above reads 32,
    the scale is the fp32 nearest to 1 / sqrt(32))."""
    what = "attention_fwd_f32"
    hd = _head_dim(head_dim, what)
    d = H * hd
    sfx = "" if hd == 64 else "_hd32"
    _chk(qkv, F32, "qkv", 2), _chk(ctx, F32, "ctx", 2)
    if mask is not None:
        _chk(mask, torch.int64, "mask", 2)
        if not mask.is_contiguous() or tuple(mask.shape) != (nseq, L):
            raise ValueError(f"{what}: mask must be contiguous int64 [nseq, L]")
    mask_p, cu_p = _layout(mask, cu, None, 0, nseq, L, what)[:2]
    if not (0 < L <= 256) or nseq < 1:
        raise ValueError(f"{what}: need nseq > 0 and 0 < L <= 256")
    rows = nseq * L if cu is None else 1
    if qkv.shape[1] != (3 if qc is None else 2) * d or not qkv.is_contiguous() or qkv.shape[0] < rows:
        raise ValueError(f"{what}: qkv must be contiguous [T, 3*H*{hd}] (CLS form: K | V, [T, 2*H*{hd}])")
    if ctx.shape[1] != d or not ctx.is_contiguous() or ctx.shape[0] < (rows if qc is None else nseq):
        raise ValueError(f"{what}: ctx must be contiguous [T, H*{hd}] (CLS form: [nseq, H*{hd}])")
    if qc is None:
        call("cldrd_attention_fwd_f32" + sfx, _p(qkv), mask_p, cu_p, _p(ctx), nseq, L, H, _stream())
    else:
        _chk(qc, F32, "qc", 2)
        if qc.shape[1] != d or qc.shape[0] < nseq:
            raise ValueError(f"{what}: qc must be [nseq, H*{hd}]")
        call("cldrd_attention_cls_fwd_f32" + sfx, _p(qc), qc.stride(0), _p(qkv), mask_p, cu_p, _p(ctx), nseq, L, H, _stream())
    return ctx


def add_rows(dst, src, M, stride=0, idx=None):
    """dst[row(m)] += src[m], row(m) = idx[m] (int32, the CLS rows of a packed batch) or m * stride: bf16 += bf16 (fp32 add, one rounding),
    fp32 += fp32 (fp32 gradient stream), or fp16 dst += fp32 src (the fp16 gradient stream)."""
    fmt = _stream_fmt(dst)
    _chk(dst, dst.dtype, "dst", 2), _chk(src, F32 if fmt else BF16, "src", 2)
    if idx is not None:
        _chk(idx, torch.int32, "idx", 1)
    call("cldrd_add_rows", _p(dst), _p(src), M, src.shape[1], stride, _p(idx), fmt, _stream())


def ln_partial_elems(T, d) -> int:
    return _lib.load().cldrd_ln_partial_blocks(T) * 3 * d


def embed_ln_fwd(ids, word, pos, type_table, gamma, beta, out, mean, rstd, T, L, eps, dropout_p=0.0, seed=0, out32=None, pos_idx=None, type_ids=None):
    """``pos_idx`` (int32 [T], packed batches): the position of every row inside its sequence; None: row % L.
    ``type_ids`` None: every row takes row 0 of ``type_table`` (fp32 [d] or [type_vocab, d]; None for DistilBERT); int32 [>= T]: per-row token
    types into the whole [type_vocab, d] table (cross-encoder pairs)."""
    _chk(ids, torch.int64, "ids")
    d = word.shape[1]
    if type_ids is not None:
        _chk(type_table, F32, "type_table", 2), _chk(type_ids, torch.int32, "type_ids", 1)
        if type_table.shape[1] != d or type_ids.numel() < T:
            raise ValueError("embed_ln_fwd: type_table must be [type_vocab, d], type_ids [>= T]")
    if out32 is not None:
        _chk(out32, F32, "out32", 2)
    if pos_idx is not None:
        _chk(pos_idx, torch.int32, "pos_idx", 1)
    call("cldrd_embed_ln_fwd", _p(ids), _p(word), _p(pos), _p(type_table), _p(type_ids), type_table.shape[0] if type_ids is not None else 0,
         _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), T, L, d, word.shape[0], eps, dropout_p, seed, _p(out32), _fmt16(out, "out"),
         _p(pos_idx), _stream())
    return out


def build_pairs(q_tok, q_lens, p_tok, p_lens, q_rows, p_rows, keep_q, keep_p, cu, T):
    """Packed ``[CLS] q' [SEP] p' [SEP]`` rows from token-cache rows (csrc/cross.hip): ``q_tok`` / ``p_tok`` [rows, stride] int32 or a
    uint16 table viewed as int16, ``*_lens`` int32 [rows], the pair arrays int32 [n], ``cu`` int32 [n + 1] with ``cu[n] == T`` (host value).
    Returns (ids int64 [T], token types int32 [T], positions int32 [T])."""
    for t, n in ((q_tok, "q_tok"), (p_tok, "p_tok")):
        if t.dtype not in (torch.int16, torch.int32) or t.dim() != 2 or not t.is_contiguous():
            raise TypeError(f"build_pairs: {n} must be a contiguous 2-d int32 (or uint16 viewed as int16) table")
        _chk(t, t.dtype, n, 2)
    for t, n in ((q_lens, "q_lens"), (p_lens, "p_lens"), (q_rows, "q_rows"), (p_rows, "p_rows"), (keep_q, "keep_q"), (keep_p, "keep_p"), (cu, "cu")):
        _chk(t, torch.int32, n, 1)
    n = q_rows.numel()
    if not (p_rows.numel() == keep_q.numel() == keep_p.numel() == n and cu.numel() == n + 1) or n < 1:
        raise ValueError("build_pairs: q_rows, p_rows, keep_q, keep_p [n], cu [n + 1], n >= 1")
    dev = q_tok.device
    ids = torch.empty(T, dtype=torch.int64, device=dev)
    types = torch.empty(T, dtype=torch.int32, device=dev)
    pos = torch.empty(T, dtype=torch.int32, device=dev)
    call("cldrd_build_pairs", _p(q_tok), _p(q_lens), q_tok.shape[1], q_tok.element_size(), _p(p_tok), _p(p_lens), p_tok.shape[1],
         p_tok.element_size(), _p(q_rows), _p(p_rows), _p(keep_q), _p(keep_p), _p(cu), n, _p(ids), _p(types), _p(pos), _stream())
    return ids, types, pos


def cls_head_fwd(cls, w1, b1, w2, b2, act):
    """Sequence-classification head on fp32 CLS rows: ``W2 act(W1 cls + b1) + b2`` -> fp32 [M, num_labels]; act "tanh" (BERT pooler) or
    "relu" (DistilBERT pre_classifier)."""
    _chk(cls, F32, "cls", 2), _chk(w1, F32, "w1", 2), _chk(b1, F32, "b1", 1), _chk(w2, F32, "w2", 2), _chk(b2, F32, "b2", 1)
    M, d = cls.shape
    nl = w2.shape[0]
    if not (cls.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()) or w1.shape != (d, d) or b1.numel() != d \
            or w2.shape[1] != d or b2.numel() != nl:
        raise ValueError("cls_head_fwd: cls [M, d], w1 [d, d], b1 [d], w2 [num_labels, d], b2 [num_labels], contiguous")
    if act not in ("tanh", "relu"):
        raise ValueError("cls_head_fwd: act is 'tanh' or 'relu'")
    out = torch.empty(M, nl, dtype=F32, device=cls.device)
    if M > 0:
        call("cldrd_cls_head_fwd", _p(cls), _p(w1), _p(b1), _p(w2), _p(b2), _p(out), M, d, nl, 0 if act == "tanh" else 1, _stream())
    return out


def embed_ln_bwd(dy, ids, word, pos, type0, gamma, mean, rstd, dword, dpos, dtype0, dgamma, dbeta, partial, T, L,
                 dropout_p=0.0, seed=0, accumulate=True, pos_idx=None, dy_branch=None):
    d = word.shape[1]
    if pos_idx is not None:
        _chk(pos_idx, torch.int32, "pos_idx", 1)
    if dy.dtype not in (BF16, F32, F16):
        raise TypeError("embed_ln_bwd: dy must be bf16, fp32 (fp32 gradient stream) or fp16 (fp16 gradient stream)")
    if dy_branch is not None and (dy.dtype not in (F32, F16) or dy_branch.dtype not in (BF16, F16) or dy_branch.shape[1] != dy.shape[1] or dy_branch.shape[0] < T
                                  or (dy.dtype == F16 and dy_branch.dtype != F16)):
        raise ValueError("embed_ln_bwd: dy_branch (bf16 or fp16 [>= T, d]) goes with an fp32 dy, an fp16 one with an fp16 dy")
    call("cldrd_embed_ln_bwd", _p(dy), _p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(mean), _p(rstd), _p(dword),
         _p(dpos), _p(dtype0), _p(dgamma), _p(dbeta), _p(partial), T, L, d, word.shape[0], dropout_p, seed,
         1 if accumulate else 0, _p(pos_idx), _stream_fmt(dy), 1 if (dy_branch is not None and dy_branch.dtype == F16) else 0, _p(dy_branch), _stream())


# ---- the deterministic mode of the embedding backward (csrc/segsum.hip): rows stored once, summed per table row in a fixed order ------
SEGMENT_CHUNK = 64          # CLDRD_SEGMENT_CHUNK of include/cldrd_hip.h: list entries per chunk of segment_sum_rows


def key_order(keys, n_keys):
    """keys int64 [T] (clamped to 0 .. n_keys - 1) -> (order int32 [T]: the stable ascending permutation of the rows by key, offsets int32
    [n_keys + 1]: the CSR starts).  Device only, no read-back, a launch sequence that depends on n_keys alone (cldrd_key_order)."""
    _chk(keys, torch.int64, "keys", 1)
    T, n_keys = keys.numel(), int(n_keys)
    if not 0 < T <= 1 << 22 or not 0 < n_keys <= 1 << 20:
        raise ValueError("key_order: 0 < T <= 2^22 keys, 0 < n_keys <= 2^20")
    dev = keys.device
    order = torch.empty(T, dtype=torch.int32, device=dev)
    offsets = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
    nbytes = int(_lib.load().cldrd_key_order_workspace(T, n_keys))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("cldrd_key_order", _p(keys), T, n_keys, _p(order), _p(offsets), _p(ws), nbytes, _stream())
    return order, offsets


def segment_sum_rows(rows, order, offsets, out, accumulate=False):
    """out[k] (+)= the sum of rows[r] over key k's list in the fixed order of cldrd_segment_sum_rows (chunks of SEGMENT_CHUNK entries summed left
    to right, chunk sums added left to right); keys without rows are left untouched.  rows fp32 [>= T, d], out fp32 [n_keys, d];
    (order, offsets) from key_order - T = order.numel() - or both None: the strided form, row r of all rows.shape[0] has key r % n_keys."""
    _chk(rows, F32, "rows", 2), _chk(out, F32, "out", 2)
    if (order is None) != (offsets is None):
        raise ValueError("segment_sum_rows: order and offsets go together")
    d, n_keys = rows.shape[1], out.shape[0]
    if out.shape[1] != d or not (rows.is_contiguous() and out.is_contiguous()):
        raise ValueError("segment_sum_rows: contiguous rows [T, d] and out [n_keys, d]")
    T = rows.shape[0]
    if order is not None:
        _chk(order, torch.int32, "order", 1), _chk(offsets, torch.int32, "offsets", 1)
        T = order.numel()
        if T > rows.shape[0] or offsets.numel() != n_keys + 1:
            raise ValueError("segment_sum_rows: order [T <= rows], offsets [n_keys + 1]")
    call("cldrd_segment_sum_rows", _p(rows), _p(order), _p(offsets), T, d, n_keys, _p(out), 1 if accumulate else 0, _stream())
    return out


# ---- k-means of embedding rows (csrc/kmeans.hip; the definition stands in include/cldrd_hip.h) -------------------------------------------
def _kmeans_centroids(op, centroids):
    _chk(centroids, F32, "centroids", 2)
    k, d = centroids.shape
    if not centroids.is_contiguous():
        raise ValueError(f"{op}: centroids must be contiguous [k, d]")
    if d % 32 or not 32 <= d <= 1024:
        raise ValueError(f"{op}: d must be a multiple of 32 with 32 <= d <= 1024, got {d}")
    if not 1 <= k <= 65536:
        raise ValueError(f"{op}: 1 <= k <= 65536, got {k}")
    return k, d


def kmeans_half_sqnorm(centroids):
    """h[j] = fp32(0.5 * sum_t centroids[j, t]^2), the sum in fp64: the constant kmeans_assign subtracts from a dot product."""
    k, d = _kmeans_centroids("kmeans_half_sqnorm", centroids)
    h = torch.empty(k, dtype=F32, device=centroids.device)
    call("cldrd_kmeans_half_sqnorm", _p(centroids), k, d, _p(h), _stream())
    return h


def kmeans_assign(x, centroids, half_sqnorm=None, best=False):
    """assign int64 [n]: the nearest centroid (L2) of every row of x fp32 [n, d] (a row pitch is allowed), the lowest index among equals -
    one launch, no [n, k] matrix in memory, and a row's result does not depend on the other rows of the launch.  ``half_sqnorm``: what
    kmeans_half_sqnorm / kmeans_update returned for these centroids (computed here when None).  ``best=True``: returns (assign, best) with
    best[i] = fp32(dot(x_i, c) - h) of the chosen centroid."""
    k, d = _kmeans_centroids("kmeans_assign", centroids)
    _chk(x, F32, "x", 2)
    n = x.shape[0]
    if x.shape[1] != d:
        raise ValueError(f"kmeans_assign: x is [n, {x.shape[1]}], centroids are [k, {d}]")
    if not k <= n <= 1 << 22:
        raise ValueError(f"kmeans_assign: k <= n <= 2^22, got n = {n}, k = {k}")
    h = kmeans_half_sqnorm(centroids) if half_sqnorm is None else _chk(half_sqnorm, F32, "half_sqnorm", 1)
    if h.numel() != k:
        raise ValueError("kmeans_assign: half_sqnorm must be [k]")
    assign = torch.empty(n, dtype=torch.int64, device=x.device)
    b = torch.empty(n, dtype=F32, device=x.device) if best else None
    call("cldrd_kmeans_assign", _p(x), x.stride(0) if n > 1 else max(x.stride(0), d), n, d, _p(centroids), _p(h), k, _p(assign), _p(b), _stream())
    return (assign, b) if best else assign


def kmeans_update(x, assign, centroids):
    """One update step, ``centroids`` in place: every non-empty cluster's centroid becomes the mean of its rows of x (contiguous fp32 [n, d]),
    the sum taken by key_order(assign) -> segment_sum_rows in that kernel's fixed order and divided once; an empty cluster keeps its row.
    Returns (half_sqnorm [k] of the new centroids, sizes int32 [k], n_empty int32 [1]) - device tensors, nothing is read back."""
    k, d = _kmeans_centroids("kmeans_update", centroids)
    _chk(x, F32, "x", 2), _chk(assign, torch.int64, "assign", 1)
    if x.shape[1] != d or not x.is_contiguous() or assign.numel() != x.shape[0]:
        raise ValueError("kmeans_update: contiguous x [n, d] (the segment sum takes no row pitch) and assign [n]")
    order, offsets = key_order(assign, k)
    sums = torch.empty(k, d, dtype=F32, device=x.device)          # rows of empty clusters stay unwritten and unread
    segment_sum_rows(x, order, offsets, sums)
    h = torch.empty(k, dtype=F32, device=x.device)
    n_empty = torch.empty(1, dtype=torch.int32, device=x.device)
    call("cldrd_kmeans_finish", _p(sums), _p(offsets), _p(centroids), _p(h), _p(n_empty), k, d, _stream())
    return h, offsets[1:] - offsets[:-1], n_empty


def embed_ln_bwd_rows(dy, ids, word, pos, type0, gamma, mean, rstd, dx_rows, dtype0, dgamma, dbeta, partial, T, L,
                      dropout_p=0.0, seed=0, accumulate=True, pos_idx=None, dy_branch=None):
    """embed_ln_bwd with ``dx_rows`` (fp32 [>= T, d]) in place of the two table gradients: row r receives what embed_ln_bwd adds into both
    tables for token r, every row written with plain stores; dgamma / dbeta / dtype0 as there, bit for bit."""
    d = word.shape[1]
    _chk(dx_rows, F32, "dx_rows", 2)
    if dx_rows.shape[1] != d or dx_rows.shape[0] < T or not dx_rows.is_contiguous():
        raise ValueError("embed_ln_bwd_rows: dx_rows is a contiguous fp32 [>= T, d]")
    if pos_idx is not None:
        _chk(pos_idx, torch.int32, "pos_idx", 1)
    if dy.dtype not in (BF16, F32, F16):
        raise TypeError("embed_ln_bwd_rows: dy must be bf16, fp32 (fp32 gradient stream) or fp16 (fp16 gradient stream)")
    if dy_branch is not None and (dy.dtype not in (F32, F16) or dy_branch.dtype not in (BF16, F16) or dy_branch.shape[1] != dy.shape[1] or dy_branch.shape[0] < T
                                  or (dy.dtype == F16 and dy_branch.dtype != F16)):
        raise ValueError("embed_ln_bwd_rows: dy_branch (bf16 or fp16 [>= T, d]) goes with an fp32 dy, an fp16 one with an fp16 dy")
    call("cldrd_embed_ln_bwd_rows", _p(dy), _p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(mean), _p(rstd), _p(dx_rows),
         _p(dtype0), _p(dgamma), _p(dbeta), _p(partial), T, L, d, word.shape[0], dropout_p, seed,
         1 if accumulate else 0, _p(pos_idx), _stream_fmt(dy), 1 if (dy_branch is not None and dy_branch.dtype == F16) else 0, _p(dy_branch), _stream())


def embed_ln_bwd_det(dy, ids, word, pos, type0, gamma, mean, rstd, dword, dpos, dtype0, dgamma, dbeta, partial, T, L,
                     dropout_p=0.0, seed=0, accumulate=True, pos_idx=None, dy_branch=None, *, word_order, pos_order, rows):
    """The deterministic form of embed_ln_bwd: the rows kernel, then the word-table sum, then the position-table sum - no float atomic, the same
    bits on every run.  ``word_order`` = key_order(ids, vocab); ``pos_order`` = key_order(positions, L) for a packed batch (``pos_idx``), None for
    a padded one (the strided form: row r sits at position r % L); ``rows``: fp32 scratch [>= T, d].  Like the atomics, the table sums are
    ADDED onto dword / dpos (zeroed by the caller, or holding the other tape of a shared tower); ``accumulate`` speaks of dgamma / dbeta / dtype0."""
    if (pos_order is None) != (pos_idx is None):
        raise ValueError("embed_ln_bwd_det: a packed batch (pos_idx) brings its position order, a padded one none")
    if word_order[0].numel() != T or (pos_order is not None and pos_order[0].numel() != T):
        raise ValueError("embed_ln_bwd_det: the orders cover the T rows of this batch")
    if dpos.shape[0] < L:
        raise ValueError("embed_ln_bwd_det: dpos holds at least L rows")
    embed_ln_bwd_rows(dy, ids, word, pos, type0, gamma, mean, rstd, rows, dtype0, dgamma, dbeta, partial, T, L, dropout_p, seed,
                      accumulate=accumulate, pos_idx=pos_idx, dy_branch=dy_branch)
    segment_sum_rows(rows, word_order[0], word_order[1], dword, accumulate=True)
    if pos_order is not None:
        segment_sum_rows(rows, pos_order[0], pos_order[1], dpos[:pos_order[1].numel() - 1], accumulate=True)
    else:
        segment_sum_rows(rows[:T], None, None, dpos[:L], accumulate=True)


# ---- variable-length packing (csrc/pack.hip) ---------------------------------------------------------------------------------------
def unpack_rows16(src_packed, dst_padded, cu, nseq, L):
    """dst[m * L + j] = j < len[m] ? src[cu[m] + j] : 0 for 16-bit rows (cu: int32 [nseq + 1] on the device)."""
    _chk(cu, torch.int32, "cu", 1)
    if src_packed.dtype not in (BF16, F16) or dst_padded.dtype != src_packed.dtype or src_packed.shape[1] != dst_padded.shape[1]:
        raise TypeError("unpack_rows16: 16-bit matrices of the same width")
    if not (src_packed.is_contiguous() and dst_padded.is_contiguous()) or dst_padded.shape[0] < nseq * L or cu.numel() < nseq + 1:
        raise ValueError("unpack_rows16: contiguous operands, dst with nseq * L rows, cu with nseq + 1 entries")
    call("cldrd_unpack_rows16", _p(src_packed), _p(dst_padded), _p(cu), nseq, L, src_packed.shape[1], _stream())
    return dst_padded


def gather_rows(src, idx, dst, n=None):
    """dst[p] = src[idx[p]] for p < n (rows of any dtype whose byte length is a multiple of 16)."""
    _chk(idx, torch.int32, "idx", 1)
    n = idx.numel() if n is None else n
    rb = src.shape[1] * src.element_size()
    if src.dtype != dst.dtype or src.shape[1] != dst.shape[1] or not (src.is_contiguous() and dst.is_contiguous()) or dst.shape[0] < n or idx.numel() < n:
        raise ValueError("gather_rows: shape mismatch")
    if n > 0:
        call("cldrd_gather_rows", _p(src), _p(idx), _p(dst), n, rb, _stream())
    return dst


def gather_i64(src, idx, n=None):
    """src[idx[:n]] for int64 ``src`` (flattened) and int32 ``idx``: the token ids of a packed batch's rows."""
    _chk(src, torch.int64, "src"), _chk(idx, torch.int32, "idx", 1)
    n = idx.numel() if n is None else n
    if not src.is_contiguous() or idx.numel() < n:
        raise ValueError("gather_i64: contiguous src, idx with at least n entries")
    out = torch.empty(n, dtype=torch.int64, device=src.device)
    if n > 0:
        call("cldrd_gather_i64", _p(src), _p(idx), _p(out), n, _stream())
    return out


def _stream_fmt(t):
    """row format code of a gradient-stream tensor: 0 bf16, 1 fp32, 2 fp16"""
    if t.dtype not in (BF16, F32, F16):
        raise TypeError(f"gradient stream tensor: expected bf16, fp32 or fp16, got {t.dtype}")
    return 1 if t.dtype == F32 else (2 if t.dtype == F16 else 0)


def layernorm_fwd(x, gamma, beta, out, mean, rstd, T, eps, cls_out=None, cls_stride=0, out32=None):
    """x bf16, or fp32 (pre-LN sum of the fp32 residual stream; then out32, optional, receives the fp32 output as well)."""
    x_f32 = 1 if x.dtype == F32 else 0
    out_f16 = _fmt16(out, "out")
    _chk(x, F32 if x_f32 else BF16, "x", 2), _chk(out, F16 if out_f16 else BF16, "out", 2), _chk(gamma, F32, "gamma", 1), _chk(beta, F32, "beta", 1)
    if out32 is not None:
        _chk(out32, F32, "out32", 2)
    d = x.shape[1]
    call("cldrd_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(out), _p(mean), _p(rstd), T, d, eps, _p(cls_out),
         cls_stride, x_f32, _p(out32), out_f16, _stream())
    return out


class LnReduceQueue:
    """Deferred LayerNorm parameter gradients of one tower: ``layernorm_bwd(..., defer=queue)`` leaves its per-block sums in a
    scratch buffer of its own and records where they go; ``flush`` reduces everything recorded so far in ONE launch
    (include/cldrd_hip.h: cldrd_ln_reduce_group) - bit-identical to the immediate form, one launch instead of one per LayerNorm."""

    def __init__(self):
        self.jobs = []

    def __len__(self):
        return len(self.jobs)

    def flush(self, accumulate=False):
        jobs, self.jobs = self.jobs, []
        if not jobs:
            return
        import ctypes as C
        n = len(jobs)
        VP, IN = C.c_void_p * n, C.c_int * n
        d = jobs[0][5]
        if any(j[5] != d for j in jobs):
            raise ValueError("LnReduceQueue: one width per queue")
        ptr = lambda t: t.data_ptr() if t is not None else None
        call("cldrd_ln_reduce_group", VP(*[j[0].data_ptr() for j in jobs]), IN(*[j[4] for j in jobs]), VP(*[ptr(j[1]) for j in jobs]),
             VP(*[ptr(j[2]) for j in jobs]), VP(*[ptr(j[3]) for j in jobs]), n, d, 1 if accumulate else 0, _stream())
        # `jobs` kept the scratch buffers alive until here (same stream: releasing them now is ordered behind the launch)


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dx_dropped, dgamma, dbeta, dbias, partial, T, dropout_p=0.0, seed=0,
                  accumulate=True, defer=None, dy_branch=None):
    """``defer`` (an LnReduceQueue): dgamma / dbeta / dbias are not produced by this call but by the queue's next ``flush``;
    ``partial`` is then a buffer of this call's own (ln_partial_elems(T, d) floats) that the queue keeps alive.
    fp32 ``dy`` = the fp32 gradient stream: ``dx`` fp32, ``dx_dropped`` (bf16, required) the MFMA operand copy; ``dy_branch`` (bf16,
    optional) is added to dy on load (the branch's data-gradient GEMM output, instead of a residual add in that GEMM's epilogue)."""
    x_f32 = 1 if x.dtype == F32 else 0
    fmt = _stream_fmt(dy)
    h16 = False                           # the 16-bit MFMA operand copy (dx_dropped) and the branch term are fp16, not bf16
    if fmt == 1:                          # fp32 gradient stream: dy and dx fp32, dx_dropped required
        if not x_f32 or dx_dropped is None:
            raise ValueError("layernorm_bwd: an fp32 dy needs fp32 x and the bf16 operand copy dx_dropped")
        h16 = dx_dropped.dtype == F16     # the all-fp16 training mode
        _chk(dx, F32, "dx", 2), _chk(dx_dropped, F16 if h16 else BF16, "dx_dropped", 2)
    elif fmt == 2:                        # fp16 gradient stream (round 5): dy, dx, dy_branch and dx_dropped fp16; dx_dropped optional
        if not x_f32:
            raise ValueError("layernorm_bwd: an fp16 dy (the fp16 gradient stream) needs fp32 x")
        h16 = True
        _chk(dx, F16, "dx", 2)
        if dx_dropped is not None:
            _chk(dx_dropped, F16, "dx_dropped", 2)
    else:
        if dy_branch is not None:
            raise ValueError("layernorm_bwd: dy_branch goes with an fp32 / fp16 dy")
        _chk(dy, BF16, "dy", 2), _chk(dx, BF16, "dx", 2)
    if dy_branch is not None:
        _chk(dy_branch, F16 if h16 else BF16, "dy_branch", 2)
        if dy_branch.shape[1] != dy.shape[1] or dy_branch.shape[0] < T:
            raise ValueError("layernorm_bwd: dy_branch must be [>= T, d]")
    _chk(x, F32 if x_f32 else BF16, "x", 2)
    d = x.shape[1]
    sums = (_p(dgamma), _p(dbeta), _p(dbias))
    if defer is not None:
        for t, nme in ((dgamma, "dgamma"), (dbeta, "dbeta"), (dbias, "dbias")):
            if t is not None:
                _chk(t, F32, nme, 1)
        if partial.numel() < ln_partial_elems(T, d):
            raise ValueError("layernorm_bwd: deferred reduction needs a partial buffer of ln_partial_elems(T, d) floats")
        sums = (None, None, None)
    call("cldrd_layernorm_bwd", _p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx), _p(dx_dropped), *sums, _p(partial), T, d, dropout_p, seed,
         1 if accumulate else 0, x_f32, fmt, 1 if h16 else 0, _p(dy_branch), _stream())
    if defer is not None:
        defer.jobs.append((partial, dgamma, dbeta, dbias, int(T), int(d)))


def colsum(x, out, partial, T, accumulate=True):
    _chk(x, BF16, "x", 2), _chk(out, F32, "out", 1)
    call("cldrd_colsum_bf16", _p(x), _p(out), _p(partial), T, x.shape[1], x.stride(0), 1 if accumulate else 0, _stream())


def scatter_cls_grad(dcls, g, R, T, stride=0, idx=None):
    """g[T, d] (bf16, fp32 or fp16: the format of the gradient stream) = 0 except rows idx[r] (int32, the CLS rows of a packed batch) or
    r * stride <- dcls[r]."""
    _chk(dcls, F32, "dcls", 2), _chk(g, g.dtype, "g", 2)
    if idx is not None:
        _chk(idx, torch.int32, "idx", 1)
    call("cldrd_scatter_cls_grad", _p(dcls), _p(g), R, dcls.shape[1], stride, _p(idx), T, _stream_fmt(g), _stream())


def score_cols(B: int, N: int, mode: int) -> int:
    """Logit columns of a row: mode 0 its own N passages, 1 then every other sample's, 2 then the next sample's (csrc/score_layout.h)."""
    return N if mode == 0 else (B * N if mode == 1 else 2 * N)


def score_fwd(q, p, logits, B, N, mode=0):
    _chk(q, F32, "q", 2), _chk(p, F32, "p", 2), _chk(logits, F32, "logits", 2)
    call("cldrd_score_fwd", _p(q), _p(p), _p(logits), B, N, q.shape[1], mode, _stream())
    return logits


def score_bwd(dlogits, q, p, dq, dp, B, N, mode=0):
    for t, n in ((dlogits, "dlogits"), (q, "q"), (p, "p"), (dq, "dq"), (dp, "dp")):
        _chk(t, F32, n, 2)
    call("cldrd_score_bwd", _p(dlogits), _p(q), _p(p), _p(dq), _p(dp), B, N, q.shape[1], mode, _stream())


COSINE_EPS = 1e-8        # of the cosine scorer and of every place that normalises embeddings (torch.nn.functional.cosine_similarity's eps)


def score_cos_fwd(q, p, logits, inv_norms, B, N, mode=0, scale=1.0, eps=COSINE_EPS):
    """logits = scale * cos(q, p) in the layout of score_fwd; inv_norms: float[B + B*N], written here and read by score_cos_bwd."""
    _chk(q, F32, "q", 2), _chk(p, F32, "p", 2), _chk(logits, F32, "logits", 2), _chk(inv_norms, F32, "inv_norms", 1)
    if inv_norms.numel() < B + B * N:
        raise ValueError(f"inv_norms: need B + B*N = {B + B * N} floats, got {inv_norms.numel()}")
    call("cldrd_score_cos_fwd", _p(q), _p(p), _p(logits), _p(inv_norms), B, N, q.shape[1], mode, float(scale), float(eps), _stream())
    return logits


def score_cos_bwd(dlogits, logits, q, p, inv_norms, dq, dp, B, N, mode=0, scale=1.0):
    for t, n in ((dlogits, "dlogits"), (logits, "logits"), (q, "q"), (p, "p"), (dq, "dq"), (dp, "dp")):
        _chk(t, F32, n, 2)
    _chk(inv_norms, F32, "inv_norms", 1)
    if inv_norms.numel() < B + B * N:
        raise ValueError(f"inv_norms: need B + B*N = {B + B * N} floats, got {inv_norms.numel()}")
    call("cldrd_score_cos_bwd", _p(dlogits), _p(logits), _p(q), _p(p), _p(inv_norms), _p(dq), _p(dp), B, N, q.shape[1], mode, float(scale),
         _stream())


def l2_normalize_rows(x, out=None, eps=COSINE_EPS):
    """out[r] = x[r] / max(||x[r]||, eps) for the rows of x [n, d] (fp32; row stride >= d); out: dense [n, d], default x itself (in place,
    which needs a dense x).  Returns out."""
    _chk(x, F32, "x", 2)
    out = x if out is None else _chk(out, F32, "out", 2)
    if out.shape != x.shape or not out.is_contiguous():
        raise ValueError("l2_normalize_rows: out must be a dense tensor of x's shape")
    if x.shape[0] == 0:
        return out
    call("cldrd_l2_normalize_rows", _p(x), x.stride(0) if x.shape[0] > 1 else x.shape[1], _p(out), x.shape[0], x.shape[1], float(eps), _stream())
    return out


LOSS_KINDS = {"kl_div": 0, "margin_mse": 1, "ranknet": 2, "lambda_mrr": 3, "weighted_pointwise": 4}
LAMBDA_SCHEMES = {None: 0, "ndcgLoss1_scheme": 1, "ndcgLoss2_scheme": 2, "lambdaRank_scheme": 3, "ndcgLoss2PP_scheme": 4, "rankNet_scheme": 5,
                  "rankNetWeightedByGTDiff_scheme": 6, "rankNetWeightedByGTDiffPowed_scheme": 7}


def loss_fwd_bwd(kind, y_pred, y_true, *, batch_weight=None, T=1.0, pad_indicator=-1.0, reduction="mean"):
    """Returns (loss_out float[2] on device = {loss, pair count}, grad [B,N])."""
    if reduction not in ("mean", "sum"):
        raise ValueError("Reduction method can be either sum or mean")
    _chk(y_pred, F32, "y_pred", 2), _chk(y_true, F32, "y_true", 2)
    if y_pred.shape != y_true.shape:
        raise ValueError("loss: y_pred and y_true must have the same shape")
    y_pred, y_true = y_pred.contiguous(), y_true.contiguous()
    B, N = y_pred.shape
    out = torch.empty(2, dtype=F32, device=y_pred.device)
    grad = torch.empty_like(y_pred)
    ws = torch.empty(2 * B, dtype=F32, device=y_pred.device)
    if batch_weight is not None:
        _chk(batch_weight, F32, "batch_weight", 1)
    call("cldrd_loss_fwd_bwd", LOSS_KINDS[kind], _p(y_pred), _p(y_true), _p(batch_weight), _p(out), _p(grad), _p(ws), B, N,
         float(T), float(pad_indicator), 1 if reduction == "mean" else 0, _stream())
    return out, grad


def _lambda_args(weighing_scheme, k, eps, sigma, mu, padded_value_indicator, reduction, reduction_log, gain):
    """The lambda_loss options, checked as the reference checks them, in the order the C entry points take them."""
    if weighing_scheme not in LAMBDA_SCHEMES:
        raise KeyError(weighing_scheme)               # the reference looks the scheme up in globals()
    if gain not in ("power", "linear"):
        raise ValueError(f"{gain} not defined.")
    if reduction_log not in ("natural", "binary"):
        raise ValueError("Reduction logarithm base can be either natural or binary")
    if reduction not in ("mean", "sum"):
        raise ValueError("Reduction method can be either sum or mean")
    return (LAMBDA_SCHEMES[weighing_scheme], 0 if k is None else int(k), float(eps), float(sigma), float(mu), float(padded_value_indicator),
            1 if reduction == "mean" else 0, 1 if reduction_log == "binary" else 0, 1 if gain == "linear" else 0)


def lambda_loss_fwd_bwd(y_pred, y_true, *, eps=1e-4, padded_value_indicator=-1, weighing_scheme=None, k=None, sigma=1.0, mu=10.0,
                        reduction="mean", reduction_log="natural", gain="power"):
    """lambda_loss of reference losses/standard_lambda_rank.py:3 -> (loss_out float[2] = {loss, pairs}, grad [B, N])."""
    largs = _lambda_args(weighing_scheme, k, eps, sigma, mu, padded_value_indicator, reduction, reduction_log, gain)
    _chk(y_pred, F32, "y_pred", 2), _chk(y_true, F32, "y_true", 2)
    if y_pred.shape != y_true.shape:
        raise ValueError("lambda_loss: y_pred and y_true must have the same shape")
    y_pred, y_true = y_pred.contiguous(), y_true.contiguous()
    B, N = y_pred.shape
    out = torch.empty(2, dtype=F32, device=y_pred.device)
    grad = torch.empty_like(y_pred)
    ws = torch.empty(2 * B, dtype=F32, device=y_pred.device)
    call("cldrd_lambda_loss_fwd_bwd", _p(y_pred), _p(y_true), _p(out), _p(grad), _p(ws), B, N, *largs, _stream())
    return out, grad


def logit_norm_reg(logits, reg_lambda, loss_out, grad, reg_out=None):
    """loss_out[0] += reg_lambda * ||logits||_2 and grad += its gradient (reference nway_listwise_1.py:348-350)."""
    _chk(logits, F32, "logits"), _chk(loss_out, F32, "loss_out", 1), _chk(grad, F32, "grad")
    if not logits.is_contiguous() or not grad.is_contiguous() or grad.numel() != logits.numel():
        raise ValueError("logit_norm_reg: logits and grad must be contiguous and of the same size")
    if reg_out is not None:
        _chk(reg_out, F32, "reg_out", 1)
    call("cldrd_logit_norm_reg", _p(logits), logits.numel(), float(reg_lambda), _p(loss_out), _p(grad), _p(reg_out), _stream())


DISTILL_KINDS = {"kl_div": 0, "margin_mse": 1}


def distill_term(kind, logits, teacher, alpha, T, loss_out, grad, term_out=None):
    """loss_out[0] += alpha * kd and grad[:, :Nt] += alpha * d kd / d logits[:, :Nt], kd = KLDiv(T) / MarginMSE of logits[:, :Nt] against
    teacher [B, Nt] (reference losses/kl_div.py, margin_mse.py); term_out[0] = kd.  Columns >= Nt of logits / grad are not touched."""
    if kind not in DISTILL_KINDS:
        raise ValueError(f"distill_term: kind must be one of {tuple(DISTILL_KINDS)}")
    _chk(logits, F32, "logits", 2), _chk(teacher, F32, "teacher", 2), _chk(loss_out, F32, "loss_out", 1), _chk(grad, F32, "grad", 2)
    if not (logits.is_contiguous() and grad.is_contiguous() and teacher.is_contiguous()) or grad.shape != logits.shape:
        raise ValueError("distill_term: logits, grad and teacher must be contiguous, grad of the shape of logits")
    B, Np = logits.shape
    if teacher.shape[0] != B or not 1 <= teacher.shape[1] <= Np:
        raise ValueError(f"distill_term: teacher must be [{B}, 1..{Np}], got {tuple(teacher.shape)}")
    if term_out is not None:
        _chk(term_out, F32, "term_out", 1)
    call("cldrd_distill_term", DISTILL_KINDS[kind], _p(logits), B, Np, _p(teacher), teacher.shape[1], float(alpha), float(T), _p(loss_out),
         _p(grad), _p(term_out), _stream())


LAMBDA_LABEL_FLAGS = {"mean": 1, "row_min": 2}          # label_flags bits of cldrd_lambda_term


def lambda_term(logits, labels, loss_out, grad, term_out=None, *, alpha=1.0, accumulate=False, neg_mean=False, row_min=False, n_rel=None,
                label_offset=0.0, eps=1e-4, padded_value_indicator=-1, weighing_scheme=None, k=None, sigma=1.0, mu=10.0,
                reduction="mean", reduction_log="natural", gain="power"):
    """The term form of lambda_loss (cldrd_lambda_term, one launch): term = lambda_loss(logits[:, :Ns], labels') with the loss parameters
    of `lambda_loss_fwd_bwd`; labels [B, Ns], Ns <= Np.  labels': columns n_rel.. replaced by their mean (``neg_mean``), the row's minimum
    subtracted (``row_min``), ``label_offset`` added, in this order, on the labels that are not padding.
    accumulate=False: loss_out = {alpha * term, pairs}, grad[:, :Ns] = alpha * d term / d logits, grad[:, Ns:] = 0;
    accumulate=True: loss_out[0] += alpha * term, grad[:, :Ns] += ...; columns >= Ns untouched.  term_out[0] = term."""
    largs = _lambda_args(weighing_scheme, k, eps, sigma, mu, padded_value_indicator, reduction, reduction_log, gain)
    _chk(logits, F32, "logits", 2), _chk(labels, F32, "labels", 2), _chk(loss_out, F32, "loss_out", 1), _chk(grad, F32, "grad", 2)
    if not (logits.is_contiguous() and grad.is_contiguous() and labels.is_contiguous()) or grad.shape != logits.shape:
        raise ValueError("lambda_term: logits, grad and labels must be contiguous, grad of the shape of logits")
    B, Np = logits.shape
    if labels.shape[0] != B or not 1 <= labels.shape[1] <= Np:
        raise ValueError(f"lambda_term: labels must be [{B}, 1..{Np}], got {tuple(labels.shape)}")
    if loss_out.numel() < 2:
        raise ValueError("lambda_term: loss_out must hold 2 floats")
    if term_out is not None:
        _chk(term_out, F32, "term_out", 1)
    Ns = labels.shape[1]
    flags = (LAMBDA_LABEL_FLAGS["mean"] if neg_mean else 0) | (LAMBDA_LABEL_FLAGS["row_min"] if row_min else 0)
    ws = torch.empty(2 * B, dtype=F32, device=logits.device)
    call("cldrd_lambda_term", _p(logits), B, Np, _p(labels), Ns, flags, Ns if n_rel is None else int(n_rel), float(label_offset), *largs,
         float(alpha), 1 if accumulate else 0, _p(loss_out), _p(grad), _p(term_out), _p(ws), _stream())


def softmax_ce(logits, labels, loss_out, grad, *, pids=None, nway=None, mode=0, temperature=1.0, pos_min=None, neg_max=0.0, reduction="mean"):
    """Softmax cross-entropy (InfoNCE) of each row's positives against its negatives (cldrd_softmax_ce, one launch; the definition is in
    include/cldrd_hip.h): loss_out = {loss, valid rows}, grad [B, Np] = d loss / d logits, every element written.  labels [B, Np] decide the
    classes: positive ``label >= pos_min`` (``pos_min=None``: the row's maximum label), negative ``label <= neg_max``, the rest neutral.
    ``pids`` (int64 [B, nway], with the scoring ``mode`` of `score_fwd`): a negative whose passage id is also behind a positive or neutral
    column of its row becomes neutral."""
    if reduction not in ("mean", "sum"):
        raise ValueError("Reduction method can be either sum or mean")
    if not float(temperature) > 0.0:
        raise ValueError("softmax_ce: temperature must be > 0")
    if pos_min is not None and not float(pos_min) > float(neg_max):
        raise ValueError("softmax_ce: pos_min must be > neg_max")
    _chk(logits, F32, "logits", 2), _chk(labels, F32, "labels", 2), _chk(loss_out, F32, "loss_out", 1), _chk(grad, F32, "grad", 2)
    if not (logits.is_contiguous() and grad.is_contiguous() and labels.is_contiguous()) or grad.shape != logits.shape or labels.shape != logits.shape:
        raise ValueError("softmax_ce: logits, grad and labels must be contiguous and of one shape")
    if loss_out.numel() < 2:
        raise ValueError("softmax_ce: loss_out must hold 2 floats")
    B, Np = logits.shape
    N = 0
    if pids is not None:
        _chk(pids, torch.int64, "pids", 2)
        N = pids.shape[1] if nway is None else int(nway)
        if mode not in (0, 1, 2) or not pids.is_contiguous() or tuple(pids.shape) != (B, N) or Np != score_cols(B, N, mode):
            raise ValueError(f"softmax_ce: pids must be contiguous [B, nway] = [{B}, {N}] with {Np} = nway | B * nway | 2 * nway logit columns "
                             f"for mode 0 | 1 | 2; got {tuple(pids.shape)}, mode {mode}")
    ws = torch.empty(2 * B, dtype=F32, device=logits.device)
    call("cldrd_softmax_ce", _p(logits), _p(labels), B, Np, _p(pids), N, int(mode) if pids is not None else 0, float(temperature),
         0.0 if pos_min is None else float(pos_min), 0 if pos_min is None else 1, float(neg_max), 1 if reduction == "mean" else 0,
         _p(loss_out), _p(grad), _p(ws), _stream())


def sqnorm_blocks() -> int:
    return _lib.load().cldrd_sqnorm_blocks()


def sqnorm_partial(g, partial, nblk):
    """partial[0:nblk] <- nblk partial sums of squares of the fp32 vector g (one piece of a norm taken in pieces, see clip_coef)."""
    call("cldrd_sqnorm_partial", _p(g), g.numel(), _p(partial), int(nblk), _stream())


def clip_coef(partial, nblk_total, max_norm, out):
    """out[3] = {norm, min(1, max_norm / (norm + 1e-6)), non-finite flag} from partial[0:nblk_total] (fixed-order fp64 sum)."""
    call("cldrd_clip_coef", _p(partial), int(nblk_total), float(max_norm), _p(out), _stream())


def grad_clip_coef(g, max_norm, partial, out):
    _chk(g, F32, "g", 1)
    call("cldrd_grad_clip_coef", _p(g), g.numel(), float(max_norm), _p(partial), _p(out), _stream())
    return out


def adamw_step(p, g, m, v, decay_flags, shadow, *, lr, beta1, beta2, eps, weight_decay, step, clip=None, shadow16=None, h16_range=None):
    """``shadow16`` (fp16, optional) receives the updated parameters ``[h16_range[0], h16_range[1])`` (``shadow16[0]`` = the first of them)."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, F32, n, 1)
    lo = hi = 0
    if shadow16 is not None:
        _chk(shadow16, F16, "shadow16", 1)
        lo, hi = int(h16_range[0]), int(h16_range[1])
        if shadow16.numel() < hi - lo:
            raise ValueError("adamw_step: shadow16 is smaller than its range")
    call("cldrd_adamw_step", _p(p), _p(g), _p(m), _p(v), _p(decay_flags), _p(shadow), p.numel(), float(lr), float(beta1),
         float(beta2), float(eps), float(weight_decay), int(step), _p(clip), _p(shadow16), lo, hi, _stream())


def cast_bf16(src, dst):
    _chk(src, F32, "src", 1), _chk(dst, BF16, "dst", 1)
    call("cldrd_cast_bf16", _p(src), _p(dst), src.numel(), _stream())


def transpose_cast_batched(src, dst, desc, tile_prefix, ndesc, total_tiles):
    call("cldrd_transpose_cast_batched", _p(src), _p(dst), _p(desc), _p(tile_prefix), ndesc, total_tiles, _stream())


def transpose_bf16_batched(src, dst, desc, tile_prefix, ndesc, total_tiles):
    """16-bit -> 16-bit transposes: bf16 or fp16 (bytes are moved, nothing is converted)."""
    if src.dtype not in (BF16, F16) or dst.dtype != src.dtype:
        raise TypeError("transpose_bf16_batched: 16-bit tensors of one format")
    _chk(src, src.dtype, "src", 1), _chk(dst, src.dtype, "dst", 1)
    call("cldrd_transpose_bf16_batched", _p(src), _p(dst), _p(desc), _p(tile_prefix), ndesc, total_tiles, _stream())


# ---------------------------------------------------------------------------------------------------- top-k search

def topk_scan_filter(Q, P, thr, counts, cand_rows, cand_scores, tiled=False):
    """Q, P: both fp16 or both bf16 (the MFMA type follows)."""
    dt = Q.dtype
    if dt not in (BF16, F16):
        raise TypeError("topk_scan_filter: Q must be fp16 or bf16")
    _chk(Q, dt, "Q", 2), _chk(P, dt, "P", 2), _chk(thr, F32, "thr", 1)
    _chk(counts, torch.int32, "counts", 1), _chk(cand_rows, torch.int32, "cand_rows", 2), _chk(cand_scores, F32, "cand_scores", 2)
    nq, d = Q.shape
    if P.shape[1] != d or not Q.is_contiguous() or not P.is_contiguous() or counts.numel() < nq + 1:
        raise ValueError("topk_scan_filter: shape mismatch (counts needs nq + 1 entries)")
    call("cldrd_topk_scan_filter", _p(Q), _p(P), nq, P.shape[0], d, _p(thr), _p(counts), _p(cand_rows), _p(cand_scores),
         cand_rows.shape[1], 1 if dt == F16 else 0, 1 if tiled else 0, _stream())


def cast_f16(src, dst, flag=None):
    """fp32 -> fp16 (RNE); flag (uint32/int32 [1], optional) |= 1 when a value does not fit fp16."""
    _chk(src, F32, "src", 1), _chk(dst, F16, "dst", 1)
    call("cldrd_cast_f16", _p(src), _p(dst), src.numel(), _p(flag), _stream())


def topk_prep_queries(q32, qh, qb, qnorm, flag):
    _chk(q32, F32, "q32", 2), _chk(qh, F16, "qh", 2), _chk(qb, BF16, "qb", 2), _chk(qnorm, F32, "qnorm", 1)
    if not (q32.is_contiguous() and qh.is_contiguous() and qb.is_contiguous()):
        raise ValueError("topk_prep_queries: operands must be contiguous")
    call("cldrd_topk_prep_queries", _p(q32), _p(qh), _p(qb), _p(qnorm), q32.shape[0], q32.shape[1], _p(flag), _stream())


def topk_thresholds(est, qnorm, pmax, d, thr, eps):
    _chk(qnorm, F32, "qnorm", 1), _chk(eps, F32, "eps", 1)
    call("cldrd_topk_thresholds", _p(est), _p(qnorm), float(pmax), int(d), _p(thr), _p(eps), qnorm.numel(), _stream())


def topk_select(counts, cand_rows, cand_scores, kk, thr, eps, rows2, n2, status, khat, exhaustive=False):
    nq = cand_rows.shape[0]
    _chk(counts, torch.int32, "counts", 1), _chk(rows2, torch.int32, "rows2", 2), _chk(n2, torch.int32, "n2", 1), _chk(status, torch.int32, "status", 1)
    if counts.numel() < nq + 1:
        raise ValueError("topk_select: counts needs nq + 1 entries")
    call("cldrd_topk_select", _p(counts), _p(cand_rows), _p(cand_scores), nq, cand_rows.shape[1], int(kk), _p(thr), _p(eps), _p(rows2),
         rows2.shape[1], _p(n2), _p(status), _p(khat), 1 if exhaustive else 0, _stream())


def _chk_search_buffers(op, nq, k, qtile, counts, cand_rows, rows2, n2, status, khat, D, I, contiguous):
    """the buffer contract both chained searches share (include/cldrd_hip.h: cldrd_flatip_search); ``contiguous``: the mode's own operands"""
    if cand_rows.shape[0] < qtile or rows2.shape[0] < qtile:
        raise ValueError(f"{op}: the candidate buffers need qtile rows")
    if counts.numel() < ((nq + qtile - 1) // qtile) * (qtile + 1) or n2.numel() < nq or status.numel() < nq or khat.numel() < nq or D.shape != (nq, k) or I.shape != (nq, k):
        raise ValueError(f"{op}: buffer sizes do not match nq / k")
    if not all(t.is_contiguous() for t in (*contiguous, D, I) if t is not None):
        raise ValueError(f"{op}: operands must be contiguous")


def flatip_search(q32, qh, thr, eps, P16, k, counts, cand_rows, cand_scores, rows2, scores2, n2, status, khat, D, I, exhaustive=False,
                  qtile=128, tiled=False, P32=None, qmu=None):
    """The whole search of one shard (include/cldrd_hip.h: cldrd_flatip_search); everything device resident, no host sync.
    ``P32`` given: fp32-row mode, the re-score reads the fp32 rows (``P16`` is the scan shadow).  ``qmu`` given instead: fp16-row mode, ``P16`` =
    fp16(p - mu) is the scan's operand and the row the re-score reads, ``qmu`` = <q, mu> (fp64 [nq], :func:`query_dot64`).
    ``tiled``: scan through the tiled kernels (cannot drop hits; the retry form for passes with status bit 4)."""
    if (P32 is None) == (qmu is None):
        raise ValueError("flatip_search: give P32 (fp32-row mode) or qmu (fp16-row mode), not both")
    P = P32 if P32 is not None else P16              # the rows the re-score reads
    _chk(q32, F32, "q32", 2), _chk(thr, F32, "thr", 1), _chk(eps, F32, "eps", 1), _chk(D, F32, "D", 2), _chk(I, torch.int32, "I", 2)
    if P32 is not None:
        _chk(P32, F32, "P32", 2)
    else:
        _chk(P16, F16, "P16", 2), _chk(qmu, torch.float64, "qmu", 1)
    nq, d = q32.shape
    if not exhaustive:
        _chk(qh, F16, "qh", 2), _chk(P16, F16, "P16", 2)
    if P.shape[1] != d or (qmu is not None and qmu.numel() < nq):
        raise ValueError("flatip_search: the rows must be [rows, d] and qmu [nq]")
    _chk_search_buffers("flatip_search", nq, k, qtile, counts, cand_rows, rows2, n2, status, khat, D, I, (q32, P, qmu))
    call("cldrd_flatip_search", _p(q32), _p(qh), _p(thr), _p(eps), _p(P16), _p(P32), _p(qmu), P.shape[0], d, nq, int(k), int(qtile), _p(counts),
         _p(cand_rows), _p(cand_scores), cand_rows.shape[1], _p(rows2), _p(scores2), rows2.shape[1], _p(n2), _p(status), _p(khat), _p(D), _p(I),
         (1 if exhaustive else 0) | (2 if tiled else 0), _stream())


def query_dot64(q32, mu):
    """<q, mu> per query in fp64 (fixed summation order) -> float64 [nq] on the device (cldrd_query_dot64)"""
    _chk(q32, F32, "q32", 2), _chk(mu, F32, "mu", 1)
    if not q32.is_contiguous() or mu.numel() != q32.shape[1]:
        raise ValueError("query_dot64: contiguous q32 [nq, d] and mu [d]")
    out = torch.empty(q32.shape[0], dtype=torch.float64, device=q32.device)
    call("cldrd_query_dot64", _p(q32), _p(mu), q32.shape[1], _p(out), q32.shape[0], _stream())
    return out


def topk_kth_largest(scores, S, kth, thr):
    _chk(scores, F32, "scores", 2), _chk(thr, F32, "thr", 1)
    call("cldrd_topk_kth_largest", _p(scores), scores.stride(0), scores.shape[0], S, int(kth), _p(thr), _stream())


def topk_rescore(q32, P, counts, cand_rows, cand_scores, qmu=None):
    """cand_scores[q, c] = exact score of row cand_rows[q, c] for c < counts[q]: fp32(<q32[q], P[row]>) for fp32 rows ``P``; for fp16 rows (the
    fp16-row mode) fp32(qmu[q] + <q32[q], P[row]>), sums in fp64, ``qmu`` = <q, mu> (fp64, :func:`query_dot64`)."""
    f16 = P.dtype == F16
    _chk(q32, F32, "q32", 2), _chk(P, F16 if f16 else F32, "P", 2)
    _chk(counts, torch.int32, "counts", 1), _chk(cand_rows, torch.int32, "cand_rows", 2), _chk(cand_scores, F32, "cand_scores", 2)
    if f16 != (qmu is not None):
        raise ValueError("topk_rescore: qmu goes with fp16 rows")
    if f16:
        _chk(qmu, torch.float64, "qmu", 1)
    if not (q32.is_contiguous() and P.is_contiguous() and cand_rows.is_contiguous() and cand_scores.is_contiguous()):
        raise ValueError("topk_rescore: operands must be contiguous")
    if P.shape[1] != q32.shape[1] or (f16 and qmu.numel() < q32.shape[0]) or counts.numel() < q32.shape[0] or cand_rows.shape != cand_scores.shape \
            or cand_rows.shape[0] < q32.shape[0]:
        raise ValueError("topk_rescore: shape mismatch")
    call("cldrd_topk_rescore", _p(q32), None if f16 else _p(P), _p(P) if f16 else None, _p(qmu), q32.shape[1], _p(counts), _p(cand_rows),
         _p(cand_scores), q32.shape[0], cand_rows.shape[1], _stream())


def topk_sort(counts, cand_rows, cand_scores, k, D, I):
    _chk(D, F32, "D", 2), _chk(I, torch.int32, "I", 2)
    call("cldrd_topk_sort", _p(counts), _p(cand_rows), _p(cand_scores), cand_rows.shape[0], cand_rows.shape[1], int(k), _p(D),
         _p(I), _stream())


def row_sqnorm_max(P32) -> float:
    out = torch.zeros(1, dtype=torch.int32, device=P32.device)
    row_sqnorm_max_into(P32, out)
    return float(out.view(torch.float32).item())


def row_sqnorm_max_into(P32, out):
    """``*out`` (int32 [1] on the device, zeroed by the caller) = max(*out, bit pattern of max_r |P32[r]|^2): the chunk-by-chunk form of
    :func:`row_sqnorm_max`, no host synchronisation"""
    _chk(P32, F32, "P32", 2), _chk(out, torch.int32, "out", 1)
    if not P32.is_contiguous():
        raise ValueError("row_sqnorm_max_into: P32 must be contiguous")
    call("cldrd_row_sqnorm_max", _p(P32), P32.shape[0], P32.shape[1], _p(out), _stream())


def gather_cast_rows(src, dst_bf16, n_out, stride):
    """dst[i] = bf16(src[i * stride]) for i < n_out; ``src`` fp32 rows, or fp16 rows (an index uploaded in fp16-row mode)"""
    f16 = src.dtype == F16
    _chk(src, F16 if f16 else F32, "src", 2), _chk(dst_bf16, BF16, "dst_bf16", 2)
    if not (src.is_contiguous() and dst_bf16.is_contiguous()) or dst_bf16.shape[1] != src.shape[1] or n_out > dst_bf16.shape[0] \
            or (n_out - 1) * stride >= src.shape[0]:
        raise ValueError("gather_cast_rows: shape mismatch")
    call("cldrd_gather_cast_rows", _p(src), 1 if f16 else 0, _p(dst_bf16), n_out, stride, src.shape[1], _stream())


def index_col_mean(P32):
    """mean row of fp32 [rows, d] (fp64 column sums in a fixed order) -> fp32 [d] (cldrd_index_col_mean)"""
    _chk(P32, F32, "P32", 2)
    rows, d = P32.shape
    mu = torch.empty(d, dtype=F32, device=P32.device)
    nbytes = int(_lib.load().cldrd_index_col_mean_workspace(rows, d))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=P32.device)
    call("cldrd_index_col_mean", _p(P32), rows, d, _p(mu), _p(ws), nbytes, _stream())
    return mu


def _chk_sample(op, sample_bf16, s_rows, d):
    """the whole shard's bf16 threshold sample an index op writes into, or None"""
    if sample_bf16 is not None:
        _chk(sample_bf16, BF16, "sample_bf16", 2)
        if int(s_rows) > sample_bf16.shape[0] or sample_bf16.shape[1] != d or not sample_bf16.is_contiguous():
            raise ValueError(f"{op}: the sample needs s_rows rows of width d")


def index_center_cast(P32, mu, P16, sample_bf16, s_stride, s_rows, flag, row0=0, cmax=None):
    """P16 = fp16(P32 - mu), sample = bf16 of every s_stride-th centred row; returns the DEVICE int32 word holding the bit pattern of
    max_r |P32[r] - mu|^2 as fp32 (cldrd_index_center_cast) - read it with ``.view(torch.float32).item()``.
    A shard attached chunk by chunk: ``P32`` / ``P16`` are rows [row0, row0 + len(P32)) of it, ``sample_bf16`` is the whole shard's sample;
    ``cmax`` (int32 [1], zeroed before the first chunk; None: a fresh one) and ``flag`` accumulate over the chunks."""
    _chk(P32, F32, "P32", 2), _chk(mu, F32, "mu", 1), _chk(P16, F16, "P16", 2)
    _chk_sample("index_center_cast", sample_bf16, s_rows, P32.shape[1])
    if P16.shape != P32.shape or mu.numel() != P32.shape[1] or not (P32.is_contiguous() and P16.is_contiguous()):
        raise ValueError("index_center_cast: P16 must be the contiguous [rows, d] slice that matches P32")
    if cmax is None:
        cmax = torch.zeros(1, dtype=torch.int32, device=P32.device)
    _chk(cmax, torch.int32, "cmax", 1)
    call("cldrd_index_center_cast", _p(P32), _p(mu), P32.shape[0], int(row0), P32.shape[1], _p(P16), _p(sample_bf16), int(s_stride), int(s_rows),
         _p(cmax), _p(flag), _stream())
    return cmax


# int8-row mode (csrc/topk_i8.hip; include/cldrd_hip.h states the definition)
I8 = torch.int8


def _chk_i8_width(d, what):
    if d <= 0 or d % 64 or d > 2048:
        raise ValueError(f"{what}: int8 rows need an embedding width that is a multiple of 64 and at most 2048, got {d}")


def index_quantize_i8(P32, mu, R8, scale, sample_bf16, s_stride, s_rows, flag, b1, c2, row0=0):
    """One fp32 chunk of a shard -> ``R8`` (int8, the matching [rows, d] slice), ``scale`` (fp32 [rows] slice), the whole shard's bf16 sample
    (rows that fall inside the chunk) and the running maxima ``b1`` / ``c2`` (int32 [1] each, zeroed before the first chunk: bit patterns of the
    fp32 values of max a_r |R8[r]|_1 and max a_r^2 |R8[r]|_2^2); ``flag`` |= 1 for a value that is not finite (cldrd_index_quantize_i8)."""
    _chk(P32, F32, "P32", 2), _chk(mu, F32, "mu", 1), _chk(R8, I8, "R8", 2), _chk(scale, F32, "scale", 1)
    _chk(b1, torch.int32, "b1", 1), _chk(c2, torch.int32, "c2", 1)
    _chk_i8_width(P32.shape[1], "index_quantize_i8")
    _chk_sample("index_quantize_i8", sample_bf16, s_rows, P32.shape[1])
    if R8.shape != P32.shape or scale.numel() != P32.shape[0] or mu.numel() != P32.shape[1] \
            or not (P32.is_contiguous() and R8.is_contiguous() and scale.is_contiguous()):
        raise ValueError("index_quantize_i8: R8 / scale must be the contiguous slices that match P32")
    call("cldrd_index_quantize_i8", _p(P32), _p(mu), P32.shape[0], int(row0), P32.shape[1], _p(R8), _p(scale), _p(sample_bf16), int(s_stride),
         int(s_rows), _p(b1), _p(c2), _p(flag), _stream())


def topk_prep_queries_i8(q32, qd, qb, sq, qnorm, flag):
    """``qd`` int8 [2, nq, d]: the digit planes h, l of the queries; ``sq`` / ``qnorm`` fp32 [nq]; ``qb`` the bf16 copy (cldrd_topk_prep_queries_i8)"""
    _chk(q32, F32, "q32", 2), _chk(qd, I8, "qd", 3), _chk(qb, BF16, "qb", 2), _chk(sq, F32, "sq", 1), _chk(qnorm, F32, "qnorm", 1)
    nq, d = q32.shape
    _chk_i8_width(d, "topk_prep_queries_i8")
    if qd.shape != (2, nq, d) or qb.shape != (nq, d) or sq.numel() != nq or qnorm.numel() != nq \
            or not (q32.is_contiguous() and qd.is_contiguous() and qb.is_contiguous()):
        raise ValueError("topk_prep_queries_i8: contiguous q32 [nq, d], qd [2, nq, d], qb [nq, d], sq / qnorm [nq]")
    call("cldrd_topk_prep_queries_i8", _p(q32), _p(qd), _p(qb), _p(sq), _p(qnorm), nq, d, _p(flag), _stream())


def topk_thresholds_i8(est, sq, qnorm, b1, cnorm, d, thr, eps):
    _chk(sq, F32, "sq", 1), _chk(qnorm, F32, "qnorm", 1), _chk(eps, F32, "eps", 1)
    if sq.numel() != qnorm.numel() or eps.numel() != qnorm.numel():
        raise ValueError("topk_thresholds_i8: sq, qnorm and eps are [nq]")
    call("cldrd_topk_thresholds_i8", _p(est), _p(sq), _p(qnorm), float(b1), float(cnorm), int(d), _p(thr), _p(eps), qnorm.numel(), _stream())


def topk_scan_i8(qd, sq, thr, R8, scale, counts, cand_rows, cand_scores):
    """Every (query, row) with scan score >= thr[query] -> the query's candidate list; ``qd`` int8 [2, nq, d] with nq <= 256, ``counts`` int32
    [nq + 1] zeroed by the caller (cldrd_topk_scan_i8)."""
    _chk(qd, I8, "qd", 3), _chk(sq, F32, "sq", 1), _chk(thr, F32, "thr", 1), _chk(R8, I8, "R8", 2), _chk(scale, F32, "scale", 1)
    _chk(counts, torch.int32, "counts", 1), _chk(cand_rows, torch.int32, "cand_rows", 2), _chk(cand_scores, F32, "cand_scores", 2)
    _, nq, d = qd.shape
    _chk_i8_width(d, "topk_scan_i8")
    if qd.shape[0] != 2 or R8.shape[1] != d or scale.numel() != R8.shape[0] or sq.numel() != nq or thr.numel() != nq or counts.numel() < nq + 1 \
            or cand_rows.shape != cand_scores.shape or cand_rows.shape[0] < nq \
            or not (qd.is_contiguous() and R8.is_contiguous() and scale.is_contiguous() and cand_rows.is_contiguous() and cand_scores.is_contiguous()):
        raise ValueError("topk_scan_i8: shape mismatch (counts needs nq + 1 entries)")
    call("cldrd_topk_scan_i8", _p(qd), nq, _p(sq), _p(thr), _p(R8), _p(scale), nq, R8.shape[0], d, _p(counts), _p(cand_rows), _p(cand_scores),
         cand_rows.shape[1], _stream())


def topk_rescore_i8(q32, R8, scale, qmu, counts, cand_rows, cand_scores):
    """cand_scores[q, c] = fp32(qmu[q] + scale[row] * <q32[q], R8[row]>) for c < counts[q], sums and product in fp64 (cldrd_topk_rescore_i8)"""
    _chk(q32, F32, "q32", 2), _chk(R8, I8, "R8", 2), _chk(scale, F32, "scale", 1), _chk(qmu, torch.float64, "qmu", 1)
    _chk(counts, torch.int32, "counts", 1), _chk(cand_rows, torch.int32, "cand_rows", 2), _chk(cand_scores, F32, "cand_scores", 2)
    _chk_i8_width(q32.shape[1], "topk_rescore_i8")
    if not (q32.is_contiguous() and R8.is_contiguous() and scale.is_contiguous() and cand_rows.is_contiguous() and cand_scores.is_contiguous()):
        raise ValueError("topk_rescore_i8: operands must be contiguous")
    if R8.shape[1] != q32.shape[1] or scale.numel() != R8.shape[0] or qmu.numel() < q32.shape[0] or counts.numel() < q32.shape[0] \
            or cand_rows.shape != cand_scores.shape or cand_rows.shape[0] < q32.shape[0]:
        raise ValueError("topk_rescore_i8: shape mismatch")
    call("cldrd_topk_rescore_i8", _p(q32), _p(R8), _p(scale), _p(qmu), q32.shape[1], _p(counts), _p(cand_rows), _p(cand_scores), q32.shape[0],
         cand_rows.shape[1], _stream())


def flatip_search_i8(q32, qd, sq, thr, eps, R8, scale, qmu, k, counts, cand_rows, cand_scores, rows2, scores2, n2, status, khat, D, I,
                     exhaustive=False, qtile=128):
    """The whole search of one shard in int8-row mode (include/cldrd_hip.h: cldrd_flatip_search_i8): the buffers and the counts / status / n2 /
    khat contract of :func:`flatip_search`; ``qd`` / ``sq`` may be None on an exhaustive search."""
    _chk(q32, F32, "q32", 2), _chk(thr, F32, "thr", 1), _chk(eps, F32, "eps", 1), _chk(D, F32, "D", 2), _chk(I, torch.int32, "I", 2)
    _chk(R8, I8, "R8", 2), _chk(scale, F32, "scale", 1), _chk(qmu, torch.float64, "qmu", 1)
    nq, d = q32.shape
    _chk_i8_width(d, "flatip_search_i8")
    if not exhaustive:
        _chk(qd, I8, "qd", 3), _chk(sq, F32, "sq", 1)
        if qd.shape != (2, nq, d) or sq.numel() != nq or not qd.is_contiguous():
            raise ValueError("flatip_search_i8: qd must be the contiguous [2, nq, d] digit planes of these queries, sq [nq]")
    if R8.shape[1] != d or scale.numel() != R8.shape[0] or qmu.numel() < nq:
        raise ValueError("flatip_search_i8: the rows must be [rows, d], their scales [rows] and qmu [nq]")
    _chk_search_buffers("flatip_search_i8", nq, k, qtile, counts, cand_rows, rows2, n2, status, khat, D, I, (q32, R8, scale, qmu))
    call("cldrd_flatip_search_i8", _p(q32), _p(qd), _p(sq), _p(thr), _p(eps), _p(R8), _p(scale), _p(qmu), R8.shape[0], d, nq, int(k), int(qtile),
         _p(counts), _p(cand_rows), _p(cand_scores), cand_rows.shape[1], _p(rows2), _p(scores2), rows2.shape[1], _p(n2), _p(status), _p(khat),
         _p(D), _p(I), 1 if exhaustive else 0, _stream())


def map_ids(I32, ids_table, id_offset):
    """row positions int32 [...] -> ids int64 [...] on the device: the id table when there is one, else position + id_offset; -1 stays -1"""
    _chk(I32, torch.int32, "I32")
    if ids_table is not None:
        _chk(ids_table, torch.int64, "ids_table", 1)
    out = torch.empty(I32.shape, dtype=torch.int64, device=I32.device)
    call("cldrd_map_ids", _p(I32), _p(ids_table), int(id_offset), _p(out), I32.numel(), _stream())
    return out


# ---------------------------------------------------------------------------------------------------- curriculum selection

def curriculum_select(qid, pid, score, count, n_rel, n_most_hard, most_hard_ranks, n_semi_hard, semi_hard_ranks, seed=0, sel_pid=None,
                      sel_score=None):
    """cldrd_curriculum_select (include/cldrd_hip.h): qid int64 [nq], pid int64 [nq, K], score fp32 [nq, K], count int32 [nq] in HBM; the
    windows are (lo, hi) pairs of 1-based inclusive teacher ranks -> (order int32 [nq, K], keep int32 [nq], sel_pid int64, sel_score fp32
    [nq, n_rel + n_most_hard + n_semi_hard]) in HBM.  ``sel_pid`` / ``sel_score``: buffers to write into (rows with keep == 0 stay as they
    are); fresh zeroed ones when not given."""
    _chk(qid, torch.int64, "qid", 1), _chk(pid, torch.int64, "pid", 2), _chk(score, F32, "score", 2), _chk(count, torch.int32, "count", 1)
    nq, K = pid.shape
    if score.shape != pid.shape or qid.shape[0] != nq or count.shape[0] != nq:
        raise ValueError("curriculum_select: qid [nq], pid [nq, K], score [nq, K], count [nq]")
    n_sel = int(n_rel) + int(n_most_hard) + int(n_semi_hard)
    if sel_pid is None:
        sel_pid = torch.zeros(nq, n_sel, dtype=torch.int64, device=pid.device)
    if sel_score is None:
        sel_score = torch.zeros(nq, n_sel, dtype=F32, device=pid.device)
    _chk(sel_pid, torch.int64, "sel_pid", 2), _chk(sel_score, F32, "sel_score", 2)
    if tuple(sel_pid.shape) != (nq, n_sel) or tuple(sel_score.shape) != (nq, n_sel):
        raise ValueError(f"curriculum_select: sel_pid / sel_score must be [{nq}, {n_sel}]")
    for t, name in ((qid, "qid"), (pid, "pid"), (score, "score"), (count, "count"), (sel_pid, "sel_pid"), (sel_score, "sel_score")):
        if not t.is_contiguous():
            raise ValueError(f"curriculum_select: {name} must be contiguous")
        if t.device != pid.device:
            raise ValueError(f"curriculum_select: {name} is on {t.device}, pid on {pid.device}")
    order = torch.empty(nq, K, dtype=torch.int32, device=pid.device)
    keep = torch.empty(nq, dtype=torch.int32, device=pid.device)
    if nq == 0:
        return order, keep, sel_pid, sel_score
    (most_lo, most_hi), (semi_lo, semi_hi) = most_hard_ranks, semi_hard_ranks
    with torch.cuda.device(pid.device):
        call("cldrd_curriculum_select", _p(qid), _p(pid), _p(score), _p(count), nq, K, int(n_rel), int(n_most_hard), int(most_lo),
             int(most_hi), int(n_semi_hard), int(semi_lo), int(semi_hi), int(seed) & ((1 << 64) - 1), _p(order), _p(keep), _p(sel_pid),
             _p(sel_score), _stream())
    return order, keep, sel_pid, sel_score


# ---------------------------------------------------------------------------------------------------- teacher score store

PAIR_SEGMENT_MAX = 2 ** 31 - 1      # entries per segment (include/cldrd_hip.h)


def _chk_flat(t, dtype, name):
    """_chk for a 1-D array by ``is_contiguous`` (an empty or one-entry tensor is contiguous whatever stride it carries)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must be on the GPU (cldrd_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous 1-D tensor")
    return t


def _pair_segment(q, p, s, op, what):
    _chk_flat(q, torch.int64, f"{what}_q"), _chk_flat(p, torch.int64, f"{what}_p"), _chk_flat(s, F32, f"{what}_s")
    if not (q.shape == p.shape == s.shape) or not (p.device == s.device == q.device):
        raise ValueError(f"{op}: {what}_q / {what}_p / {what}_s are one segment: one length, one device")
    if q.numel() > PAIR_SEGMENT_MAX:
        raise ValueError(f"{op}: a segment holds at most 2^31 - 1 entries")


def pair_lookup(seg_q, seg_p, seg_s, qid, starts, pid, score_out=None, hit=None):
    """cldrd_pair_lookup (include/cldrd_hip.h): the pairs of the CSR batch qid int64 [nq] / starts int64 [nq + 1] / pid int64 [total]
    searched in the segment (seg_q, seg_p, seg_s) -> (score_out fp32 [total], hit uint8 [total]).  A found pair gets the stored score bits
    and hit 1, a missed one leaves both as they were: pass the outputs of one call to the next to search several segments (fresh zeroed ones
    when not given).  Everything in HBM."""
    _pair_segment(seg_q, seg_p, seg_s, "pair_lookup", "seg")
    _chk_flat(qid, torch.int64, "qid"), _chk_flat(starts, torch.int64, "starts"), _chk_flat(pid, torch.int64, "pid")
    nq, total = qid.shape[0], pid.shape[0]
    if starts.shape[0] != nq + 1:
        raise ValueError("pair_lookup: qid [nq], starts [nq + 1], pid [total]")
    if score_out is None:
        score_out = torch.zeros(total, dtype=F32, device=pid.device)
    if hit is None:
        hit = torch.zeros(total, dtype=torch.uint8, device=pid.device)
    _chk_flat(score_out, F32, "score_out"), _chk_flat(hit, torch.uint8, "hit")
    if score_out.shape[0] != total or hit.shape[0] != total:
        raise ValueError(f"pair_lookup: score_out / hit must be [{total}]")
    for t, name in ((seg_q, "seg"), (qid, "qid"), (starts, "starts"), (score_out, "score_out"), (hit, "hit")):
        if t.device != pid.device:
            raise ValueError(f"pair_lookup: {name} is on {t.device}, pid on {pid.device}")
    if nq == 0 or total == 0 or seg_q.shape[0] == 0:
        return score_out, hit
    with torch.cuda.device(pid.device):
        call("cldrd_pair_lookup", _p(seg_q), _p(seg_p), _p(seg_s), seg_q.shape[0], _p(qid), _p(starts), _p(pid), nq, total, _p(score_out),
             _p(hit), _stream())
    return score_out, hit


def pair_merge(a_q, a_p, a_s, b_q, b_p, b_s):
    """cldrd_pair_merge (include/cldrd_hip.h): two segments with no key in common -> the merged segment (q, p, s) of na + nb entries, in
    HBM.  ``ValueError`` when a key occurs in both (the flag is read here: one synchronisation).  An empty side: a copy of the other,
    no launch."""
    _pair_segment(a_q, a_p, a_s, "pair_merge", "a"), _pair_segment(b_q, b_p, b_s, "pair_merge", "b")
    if a_q.device != b_q.device:
        raise ValueError(f"pair_merge: a is on {a_q.device}, b on {b_q.device}")
    na, nb = a_q.shape[0], b_q.shape[0]
    if na + nb > PAIR_SEGMENT_MAX:
        raise ValueError("pair_merge: a segment holds at most 2^31 - 1 entries (na + nb)")
    if na == 0 or nb == 0:
        q, p, s = (b_q, b_p, b_s) if na == 0 else (a_q, a_p, a_s)
        return q.clone(), p.clone(), s.clone()
    dev = a_q.device
    out_q = torch.empty(na + nb, dtype=torch.int64, device=dev)
    out_p = torch.empty(na + nb, dtype=torch.int64, device=dev)
    out_s = torch.empty(na + nb, dtype=F32, device=dev)
    dup = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("cldrd_pair_merge", _p(a_q), _p(a_p), _p(a_s), na, _p(b_q), _p(b_p), _p(b_s), nb, _p(out_q), _p(out_p), _p(out_s), _p(dup),
             _stream())
    if int(dup.item()):
        raise ValueError("pair_merge: a key occurs in both inputs")
    return out_q, out_p, out_s


# ---------------------------------------------------------------------------------------------------- merge of shard lists

def merge_topk_host(shard_D, shard_I, k, nthreads=0):
    """Host k-way merge (include/cldrd_hip.h: cldrd_merge_topk) of per-shard lists: numpy float32 [nq, k_in] / int64 [nq, k_in] per shard
    -> (D float32 [nq, k], I int64 [nq, k]).  Native host threads; no GPU work."""
    import ctypes as C
    import numpy as np
    world = len(shard_D)
    if world == 0 or len(shard_I) != world:
        raise ValueError("merge_topk_host: one score list and one id list per shard")
    Ds = [np.ascontiguousarray(d, dtype=np.float32) for d in shard_D]
    Is = [np.ascontiguousarray(i, dtype=np.int64) for i in shard_I]
    nq, k_in = Ds[0].shape
    if any(d.shape != (nq, k_in) for d in Ds) or any(i.shape != (nq, k_in) for i in Is):
        raise ValueError("merge_topk_host: every shard list must be [nq, k_in]")
    k = int(k)
    D = np.empty((nq, k), dtype=np.float32)
    I = np.empty((nq, k), dtype=np.int64)
    if nq == 0:
        return D, I
    VP = C.c_void_p * world
    call("cldrd_merge_topk", VP(*[d.ctypes.data for d in Ds]), VP(*[i.ctypes.data for i in Is]), world, nq, k_in, k, D.ctypes.data,
         I.ctypes.data, int(nthreads))
    return D, I


def merge_topk_device(scores, ids, k):
    """Device merge (cldrd_merge_topk_device): scores fp32 [world, nq, k_in], ids int64 [world, nq, k_in] in HBM -> (D fp32 [nq, k],
    I int64 [nq, k]) in HBM; world * k_in <= 8192, k <= world * k_in."""
    _chk(scores, F32, "scores", 3), _chk(ids, torch.int64, "ids", 3)
    if scores.shape != ids.shape or not scores.is_contiguous() or not ids.is_contiguous():
        raise ValueError("merge_topk_device: contiguous [world, nq, k_in] scores and ids")
    world, nq, k_in = scores.shape
    k = int(k)
    D = torch.empty(nq, k, dtype=F32, device=scores.device)
    I = torch.empty(nq, k, dtype=torch.int64, device=scores.device)
    if nq == 0:
        return D, I
    nbytes = int(_lib.load().cldrd_merge_topk_device_workspace(world, nq, k_in, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    call("cldrd_merge_topk_device", _p(scores), _p(ids), world, nq, k_in, k, _p(D), _p(I), _p(ws), nbytes, _stream())
    return D, I
