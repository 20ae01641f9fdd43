"""Strided and sliced operands of the 16-bit NT GEMM and the weight gradient, from the host (no GPU).

Two halves.  With every launch stubbed (the stubs of tests/test_encoder_dryrun.py, built locally): ``ops.gemm_nt`` refuses a GELU tape that does
not share ``out``'s row pitch - the C ABI gives ``preact`` / ``gelu_pre`` no leading dimension of their own, the kernels index them with ``ldc`` -
and a bias that is not [N], and hands the row pitches and offset base pointers of strided views to ``cldrd_gemm_nt16`` unchanged.  With the real
library and fake pointers: the entry points refuse a misaligned bias / tape pointer and a bad weight-gradient row pitch in front of any HIP call
(as tests/test_gemm_plan_host.py does for the fp16 residual)."""
import pytest
import torch

from cldrd_amd import _lib, hip_ops as ops

BF16, F32 = torch.bfloat16, torch.float32
M, N, K = 70, 136, 128
P = 64                                      # any non-null, 16-byte aligned "pointer"


@pytest.fixture
def calls(monkeypatch):
    """Every launch recorded instead of made, the device check of the argument validators lifted: [(entry point, argument tuple)]."""
    _lib.load()
    recorded = []

    def chk(t, dtype, name, dim=None):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor")
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        if dim is not None and t.dim() != dim:
            raise ValueError(f"{name}: expected {dim} dims, got {t.dim()}")
        if t.stride(-1) != 1:
            raise ValueError(f"{name}: last dim must be contiguous")
        return t
    monkeypatch.setattr(ops, "_chk", chk)
    monkeypatch.setattr(ops, "call", lambda name, *a: recorded.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return recorded


def _operands():
    return torch.zeros(M, K, dtype=BF16), torch.zeros(N, K, dtype=BF16), torch.zeros(M, N, dtype=BF16), torch.zeros(N, dtype=F32)


def test_gemm_nt_accepts_a_tape_of_the_pitch_of_out(calls):
    """the control of the refusals below: the same calls with a well-formed tape and bias go through to the launch"""
    A, B, out, bias = _operands()
    ops.gemm_nt(A, B, out, bias=bias, preact=torch.zeros(M, N, dtype=BF16), act=3)
    ops.gemm_nt(A, B, out, gelu_pre=torch.zeros(M + 2, N, dtype=BF16), act=2)
    wide_c, wide_t = torch.zeros(M, 3 * N, dtype=BF16), torch.zeros(M, 3 * N, dtype=BF16)
    ops.gemm_nt(A, B, wide_c[:, N:2 * N], bias=bias, preact=wide_t[:, N:2 * N], act=3)          # both strided, equal pitch
    assert [n for n, _ in calls] == ["cldrd_gemm_nt16"] * 3
    assert calls[2][1][8] == 3 * N and calls[2][1][12] == wide_t.data_ptr() + 2 * N


@pytest.mark.parametrize("case", ["preact_pitch", "preact_rows", "gelu_pre_width", "bias_length"])
def test_gemm_nt_refuses_a_tape_or_bias_the_kernels_would_index_out_of_place(calls, case):
    A, B, out, bias = _operands()
    kw = {}
    if case == "preact_pitch":              # right shape, but rows 3 N apart while out's are N apart
        kw.update(bias=bias, preact=torch.zeros(M, 3 * N, dtype=BF16)[:, N:2 * N], act=3)
    if case == "preact_rows":
        kw.update(bias=bias, preact=torch.zeros(M - 1, N, dtype=BF16), act=3)
    if case == "gelu_pre_width":
        kw.update(gelu_pre=torch.zeros(M, N + 8, dtype=BF16), act=2)
    if case == "bias_length":
        kw.update(bias=torch.zeros(N + 8, dtype=F32))
    what = {"preact_pitch": "preact", "preact_rows": "preact", "gelu_pre_width": "gelu_pre", "bias_length": "bias"}[case]
    with pytest.raises(ValueError, match=f"gemm_nt: {what} must be"):
        ops.gemm_nt(A, B, out, **kw)
    assert calls == []


def test_gemm_nt_forwards_row_pitches_and_offset_base_pointers_unchanged(calls):
    """A = rows of a wider buffer (the CLS rows), B = a column slice (wt[:, d:]), C = a column slice, the fp32 residual = rows of a buffer of
    a fourth pitch: lda, ldb, ldc, ldr reach the C entry point as the views' stride(0), the pointers as their data_ptr()."""
    Aw, Bw = torch.zeros(M + 3, 5 * K, dtype=BF16), torch.zeros(N, 3 * K, dtype=BF16)
    Cw, Rw = torch.zeros(M + 3, 3 * N, dtype=F32), torch.zeros(M + 3, 7 * N, dtype=F32)
    A, B, out, res = Aw[:M, :K], Bw[:, K:2 * K], Cw[:, N:2 * N], Rw[:M, :N]
    ops.gemm_nt(A, B, out, M, bias=torch.zeros(N, dtype=F32), residual=res)
    (name, a), = calls
    assert name == "cldrd_gemm_nt16"
    assert a[3:9] == (M, N, K, 5 * K, 3 * K, 3 * N) and a[11] == 7 * N
    assert a[0] == Aw.data_ptr() and a[1] == Bw.data_ptr() + 2 * K and a[2] == Cw.data_ptr() + 4 * N and a[10] == Rw.data_ptr()
    assert a[18:20] == (1, 1)               # fp32 out, fp32 residual


def _refused(fn, *args):
    lib = _lib.load()
    lib.cldrd_set_tuning(None, 0)           # leaves "set_tuning: null key" behind: the message read afterwards is the call's own
    assert getattr(lib, fn)(*args) != 0
    return lib.cldrd_last_error().decode()


@pytest.mark.parametrize("which", ["bias", "preact", "gelu_pre"])
def test_gemm_nt16_refuses_a_misaligned_bias_or_tape_pointer_before_any_launch(which):
    """bias, preact and gelu_pre are read and written with 16-byte vector accesses like A, B, C and the residual"""
    bias, preact, gelu_pre = (P + 4 if which == n else None for n in ("bias", "preact", "gelu_pre"))
    act = {"bias": 0, "preact": 3, "gelu_pre": 2}[which]
    msg = _refused("cldrd_gemm_nt16", P, P, P, 64, 64, 64, 64, 64, 64, bias, None, 0, preact, gelu_pre, act, 1.0, 0.0, 7, 0, 0, ops.FMT_BF16,
                   None, None, None, None, None, 0, None)
    assert msg == "gemm_nt: bias / preact / gelu_pre must be 16-byte aligned"


@pytest.mark.parametrize("lda,message", [(2 ** 25, "wgrad: row pitch too large"), (132, "wgrad: lda/ldb must be multiples of 8")])
def test_wgrad16_refuses_a_bad_row_pitch_before_any_launch(lda, message):
    """the weight-gradient kernels keep 32-bit byte offsets of up to 72 token rows and fetch 16 bytes per lane"""
    assert _refused("cldrd_wgrad16", P, P, P, None, 130, 128, 128, lda, 128, None, 0, 0, None) == message
