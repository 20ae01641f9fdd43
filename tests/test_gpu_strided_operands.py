"""Strided and sliced operands of the 16-bit NT GEMM (cldrd_gemm_nt16) and the weight-gradient kernels (cldrd_wgrad16 / cldrd_wgrad_group).

The encoder hands these kernels non-contiguous operands on every training step (encoder.py, _last_layer_cls_fwd / _last_layer_cls_bwd): the CLS
rows of a padded batch as A, as fp32 residual and as the weight gradient's X (row pitch L * d), column slices of a fused weight as B (ldb = 3 d,
offset base pointer), row slices of a fused gradient as dW / dbias.  The principle of every case here: A PITCH MUST CHANGE NOTHING.  The same
arithmetic runs twice, on contiguous copies (the control) and on strided views of wider buffers, and every output - C and the written GELU tape -
must be equal bit for bit.  The control is also compared with a float64 statement of the flavour (expressions and tolerances of
test_gpu_kernels.py: test_gemm_nt_epilogues / test_gemm_nt_ring_flavours_partial_tiles / test_wgrad), so the pair cannot be wrong together.

Everything outside the used window of an input buffer is NaN (padding columns, rows >= M): a read beyond a row's K or N elements that reaches an
output shows up.  Output and tape buffers are prefilled with 7.0 and everything outside the written window must still hold it afterwards.

Each of the seven dispatch families of the NT GEMM has its own operand staging, and three epilogue forms (the tile epilogue, splitk_finish_kernel,
the ring's fp32 epilogue) compute m * ldc and m * ldr on their own: every family is reached at the smallest shape that has a ragged M tile and more
than one N tile, and its launch plan is pinned through cldrd_gemm_nt_splitk_workspace under the tuning state in force."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from cldrd_amd import hip_ops as ops
from oracle import dropout_ref as DRo

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAN = float("nan")
SENTINEL = 7.0
P_DROP, SEED = 0.1, (5 << 32) | 77           # a seed with bits above 2^32
TUNING_DEFAULTS = {"gemm_splitk": 0, "gemm_nt64": 1}

# family -> ((M, N, K), tuning state, K ranges whose fp32 partials the workspace holds (0: one launch)).  From csrc/gemm_nt.hip (nt64_splits,
# splitk_choice, nt_plan) and csrc/gemm_nt_ring.hip (cldrd_gemm_nt_ring_dispatch):
#   tile64          2 x 3 tiles of 64 x 64, K <= 1024: one launch
#   tile64_splitk   6 tiles, 32 K tiles: min(256 / 6, 32 / 8) = 4 ranges
#   tile128_splitk  a forced split count takes the 64 x 64 kernel out; 8 K tiles, 3 ranges forced
#   tile128         "never split": the 128 x 128 kernel in one pass (1 x 2 tiles, 70 of 128 rows)
#   ring192 / 256   M >= 1024 and N a multiple of 192 / 256: 256-row ring tiles, the last with 6 of 256 rows
#   tile128_large_m M >= 1024, N a multiple of neither: the ring declines, 9 x 2 tiles of 128 x 128
FAMILIES = {
    "tile64": ((70, 136, 128), {}, 0),
    "tile64_splitk": ((70, 136, 2048), {}, 4),
    "tile128_splitk": ((70, 136, 512), {"gemm_splitk": 3}, 3),
    "tile128": ((70, 136, 128), {"gemm_splitk": 1}, 0),
    "ring192": ((1030, 192, 128), {}, 0),
    "ring256": ((1030, 256, 128), {}, 0),
    "tile128_large_m": ((1030, 136, 64), {}, 0),
}
RING = ("ring192", "ring256")
# which operand groups are strided views; only one in each of the first four, so a failure names its operand
LAYOUTS = {"A": {"A"}, "B": {"B"}, "residual": {"res"}, "C_tape": {"ctape"}, "all": {"A", "B", "res", "ctape"}}

BF16_FLAVOURS = ["plain", "bias_gelu_dpre", "gelugrad_d", "res16", "bias_drop_res32_f32", "ln_res32_f32"]
# fp16 operands: fp16 C; bf16 C (the QKV projection); fp32 residual stream; FFN1 with an fp16 tape
F16_FLAVOURS = ["plain", "bias_c_bf16", "bias_res32_f32", "bias_gelu_dpre"]
# the ring builds only EpiF16Ring for fp16 operands (gemm_epilogue.h): the forward FFN flavours
F16_RING_FLAVOURS = ["bias_gelu", "bias_gelu_dpre", "ln_res32_f32", "drop_ln_res32_f32"]


def close(got, ref, rtol, atol, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    bad = int((~(err <= atol + rtol * ref.abs())).sum())          # a NaN counts as off
    assert bad == 0, f"{what}: {bad}/{err.numel()} off, max err {err.max().item():.4e} (ref max {ref.abs().max().item():.3e})"


class Problem:
    """Inputs of one (family, operand format), made once and never written: contiguous device tensors and their float64 copies on the host."""

    def __init__(self, family, f16):
        (M, N, K), _, _ = FAMILIES[family]
        dt = F16 if f16 else BF16
        g = torch.Generator().manual_seed(1000 * sorted(FAMILIES).index(family) + (1 if f16 else 0))
        r = lambda *shape: torch.randn(*shape, generator=g)
        self.M, self.N, self.K, self.dt = M, N, K, dt
        host = {"A": (r(M, K) * 0.5).to(dt), "B": (r(N, K) * 0.5).to(dt), "bias": r(N), "res16": r(M, N).to(BF16), "res32": r(M, N),
                "gp": r(M, N).to(dt), "s32": r(M, N) * 2.0 + 0.5, "gamma": 1 + 0.1 * r(N), "beta": 0.1 * r(N)}
        host["mean"] = host["s32"].mean(1)
        host["rstd"] = 1.0 / torch.sqrt(host["s32"].var(1, unbiased=False) + 1e-12)
        self.h = {k: v.double() for k, v in host.items()}
        self.d = {k: v.to(DEV) for k, v in host.items()}
        self.base = self.h["A"] @ self.h["B"].T
        self.keep = torch.from_numpy(DRo.keep_mask(SEED, P_DROP, M, N))

    @functools.lru_cache(maxsize=None)
    def reference(self, flavour):
        """(C, tape or None) of the flavour in float64"""
        h, x, tape = self.h, self.base, None
        if "bias" in flavour or "ln" in flavour:
            x = x + h["bias"]
        if "gelu_dpre" in flavour:
            tape = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        if "bias_gelu" in flavour:
            x = torch.nn.functional.gelu(x)
        if flavour == "gelugrad_d":
            x = x * h["gp"]
        if "drop" in flavour:
            x = torch.where(self.keep, x / (1 - P_DROP), torch.zeros((), dtype=torch.float64))
        if flavour == "res16":
            x = x + h["res16"]
        if "ln_res32" in flavour:
            x = x + (h["s32"] - h["mean"][:, None]) * h["rstd"][:, None] * h["gamma"] + h["beta"]
        elif "res32" in flavour:
            x = x + h["res32"]
        return x, tape


@functools.lru_cache(maxsize=None)
def problem(family, f16):
    return Problem(family, f16)


def window(t, rows, width, col0, whole_rows=False):
    """``t`` as a window at column ``col0`` of a NaN-filled [rows, width] buffer (``whole_rows``: the view keeps every row of the buffer)"""
    wide = torch.full((rows, width), NAN, dtype=t.dtype, device=DEV)
    wide[:t.shape[0], col0:col0 + t.shape[1]].copy_(t)
    return wide[:, col0:col0 + t.shape[1]] if whole_rows else wide[:t.shape[0], col0:col0 + t.shape[1]]


def sentinel_window(M, N, dtype, strided):
    """(buffer, view the kernel writes): [M + 3, N] contiguous, or columns N .. 2 N of [M + 3, 3 N]"""
    wide = torch.full((M + 3, 3 * N if strided else N), SENTINEL, dtype=dtype, device=DEV)
    return wide, (wide[:, N:2 * N] if strided else wide)


def assert_rest_untouched(wide, view, M, what):
    outside = torch.ones(wide.shape, dtype=torch.bool, device=DEV)
    c0 = view.storage_offset() - wide.storage_offset()
    outside[:M, c0:c0 + view.shape[1]] = False
    assert bool((wide[outside] == SENTINEL).all()), f"{what}: written outside [:M, window]"


def launch(p, flavour, strided):
    """One gemm_nt call of the flavour; ``strided``: the operand groups given as views of wider buffers.  -> (C buffer, C view, tape buffer, tape view)"""
    M, N, K, d = p.M, p.N, p.K, p.d
    A = window(d["A"], M + 3, 5 * K, 0) if "A" in strided else d["A"]
    B = window(d["B"], N, 3 * K, K) if "B" in strided else d["B"]
    res = lambda t: window(t, M + 3, 3 * N, 0) if "res" in strided else t
    ct = "ctape" in strided
    kw, out_dtype, tape_wide, tape = {}, p.dt, None, None
    if "bias" in flavour or "ln" in flavour:
        kw["bias"] = d["bias"]
    if flavour == "bias_c_bf16":
        out_dtype = BF16
    if flavour == "bias_gelu":
        kw["act"] = 1
    if flavour == "bias_gelu_dpre":
        tape_wide, tape = sentinel_window(M, N, p.dt, ct)
        kw.update(preact=tape, act=3)
    if flavour == "gelugrad_d":           # the tape shares C's pitch: strided with C, never alone
        kw.update(gelu_pre=window(d["gp"], M + 3, 3 * N, N, whole_rows=True) if ct else d["gp"], act=2)
    if flavour == "res16":
        kw["residual"] = res(d["res16"])
    if "drop" in flavour:
        kw.update(dropout_p=P_DROP, seed=SEED)
    if "ln_res32" in flavour:
        kw.update(residual=res(d["s32"]), residual_ln=(d["mean"], d["rstd"], d["gamma"], d["beta"]))
        out_dtype = F32
    elif "res32" in flavour:
        kw["residual"] = res(d["res32"])
        out_dtype = F32
    wide, out = sentinel_window(M, N, out_dtype, ct)
    ops.gemm_nt(A, B, out, M, **kw)
    return wide, out, tape_wide, tape


def run_case(family, flavour, layout, f16):
    (M, N, K), tuning, ranges = FAMILIES[family]
    p = problem(family, f16)
    lib = ops._lib.load()
    try:
        for key, value in tuning.items():
            ops.set_tuning(key, value)
        # the launch plan of the shape under this tuning state: K ranges of fp32 partials (or none)
        assert lib.cldrd_gemm_nt_splitk_workspace(M, N, K) == ranges * M * N * 4, f"{family}: the launch plan moved"
        control = launch(p, flavour, set())
        strided = launch(p, flavour, LAYOUTS[layout])
        torch.cuda.synchronize()
    finally:
        for key, value in TUNING_DEFAULTS.items():
            ops.set_tuning(key, value)
    ref, ref_tape = p.reference(flavour)
    what = f"{family} {flavour} {'fp16' if f16 else 'bf16'}"
    (cw, c, ctw, ctape), (sw, s, stw, stape) = control, strided
    if c.dtype == F32:
        close(c[:M], ref, 2e-5, 2e-4 * math.sqrt(K), what + " (contiguous) against float64")
    else:
        close(c[:M], ref, 1 / 128, 2e-2, what + " (contiguous) against float64")
    assert torch.equal(s[:M], c[:M]), f"{what}, {layout} strided: C differs, max {(s[:M].double() - c[:M].double()).abs().max().item():.4e}"
    assert_rest_untouched(cw, c, M, what + " C (contiguous)")
    assert_rest_untouched(sw, s, M, f"{what} C ({layout} strided)")
    if ref_tape is not None:
        close(ctape[:M], ref_tape, 1 / 128, 2e-2, what + " tape (contiguous) against float64")
        assert torch.equal(stape[:M], ctape[:M]), f"{what}, {layout} strided: the tape differs"
        assert_rest_untouched(ctw, ctape, M, what + " tape (contiguous)")
        assert_rest_untouched(stw, stape, M, f"{what} tape ({layout} strided)")


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("flavour", BF16_FLAVOURS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemm_nt_bf16_strided_operands_change_nothing(family, flavour, layout):
    run_case(family, flavour, layout, False)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("family,flavour", [(fam, fl) for fam in FAMILIES for fl in (F16_RING_FLAVOURS if fam in RING else F16_FLAVOURS)])
def test_gemm_nt_fp16_strided_operands_change_nothing(family, flavour, layout):
    run_case(family, flavour, layout, True)


def test_gemm_nt_large_pitch_a_takes_the_128x128_kernel_with_64_bit_addresses():
    """A = 1024 rows 2^21 elements apart: M * lda * 2 = 2^32 bytes >= 4.0e9, so the ring (32-bit LDS-DMA offsets) declines and the 128 x 128
    kernel, whose staging forms 64-bit row addresses, takes the call; the last row starts 4 GiB - 4 MiB behind the first."""
    M, N, K, pitch = 1024, 256, 64, 2 ** 21
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        print(f"large-pitch case skipped: {free / 2 ** 30:.1f} GiB of device memory free, 6 GiB wanted")
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, 6 GiB wanted")
    assert M * pitch * 2 >= 4.0e9 and ops._lib.load().cldrd_gemm_nt_splitk_workspace(M, N, K) == 0
    g = torch.Generator().manual_seed(21)
    A, B = (torch.randn(M, K, generator=g) * 0.5).to(BF16), (torch.randn(N, K, generator=g) * 0.5).to(BF16)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    buf = torch.empty(M * pitch, dtype=BF16, device=DEV)           # 4 GiB, never filled: only the window is written
    Aw = buf.view(M, pitch)[:, :K]
    Aw.copy_(A)
    assert Aw.stride(0) == pitch and Aw[M - 1].data_ptr() - buf.data_ptr() == (M - 1) * pitch * 2
    wide = torch.full((M + 3, N), SENTINEL, dtype=F32, device=DEV)
    ops.gemm_nt(Aw, B.to(DEV), wide, M, bias=bias.to(DEV), residual=res.to(DEV))
    control = torch.empty(M, N, dtype=F32, device=DEV)
    ops.gemm_nt(A.to(DEV), B.to(DEV), control, M, bias=bias.to(DEV), residual=res.to(DEV))       # contiguous: the ring kernel
    torch.cuda.synchronize()
    ref = A.double() @ B.double().T + bias.double() + res.double()
    close(wide[:M], ref, 2e-5, 2e-4 * math.sqrt(K), "large-pitch A against float64")
    close(control, ref, 2e-5, 2e-4 * math.sqrt(K), "contiguous A against float64")
    assert bool((wide[M:] == SENTINEL).all())
    del Aw, buf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ weight gradient
# One shape per tile form of wgrad_tile_group (csrc/gemm_tn.hip); M = 130: two 64-token K tiles and a 2-row tail fetched beside the zero
# page, M = 128: whole K tiles only.
WGRAD_TILES = {(128, 128): (128, 128), (256, 128): (256, 128), (256, 192): (256, 192)}


def wgrad_tile(lib, probs):
    import ctypes as C
    n = len(probs)
    IN = C.c_int * n
    chunks, info, model = (C.c_int * (4 * n))(), (C.c_int * 8)(), (C.c_double * 2)()
    assert lib.cldrd_wgrad_plan(IN(*[p[0] for p in probs]), IN(*[p[1] for p in probs]), IN(*[p[2] for p in probs]), n, 0, chunks, info, model) == 0
    return info[0], info[1]


@functools.lru_cache(maxsize=None)
def wgrad_problem(M, N1, N2, f16, seed):
    """(dY, X) on the device, (dW, dbias) of dY^T X in float64"""
    g = torch.Generator().manual_seed(seed)
    dt = F16 if f16 else BF16
    dY, X = torch.randn(M, N1, generator=g).to(dt), torch.randn(M, N2, generator=g).to(dt)
    return dY.to(DEV), X.to(DEV), dY.double().T @ X.double(), dY.double().sum(0)


def wgrad_outputs(N1, N2, sliced):
    """(dW buffer, dW, dbias buffer, dbias): the middle third of a [3 N1, N2] tensor and of a [3 N1] vector, or tensors of their own"""
    Wb = torch.full((3 * N1 if sliced else N1, N2), SENTINEL, dtype=F32, device=DEV)
    bb = torch.full((3 * N1 if sliced else N1,), SENTINEL, dtype=F32, device=DEV)
    return (Wb, Wb[N1:2 * N1], bb, bb[N1:2 * N1]) if sliced else (Wb, Wb, bb, bb)


def wgrad_check(control, strided, refW, refb, M, N1, accumulate, what):
    (_, cW, _, cb), (sWb, sW, sbb, sb) = control, strided
    base = SENTINEL if accumulate else 0.0
    close(cW, base + refW, 1e-4, 1e-4 * math.sqrt(M), what + " dW (contiguous) against float64")
    close(cb, base + refb, 1e-4, 1e-4 * math.sqrt(M), what + " dbias (contiguous) against float64")
    assert torch.equal(sW, cW), f"{what}: dW differs, max {(sW - cW).abs().max().item():.4e}"
    assert torch.equal(sb, cb), f"{what}: dbias differs"
    for buf in (sWb, sbb):          # the neighbouring thirds of the fused gradient
        assert bool((buf[:N1] == SENTINEL).all()) and bool((buf[2 * N1:] == SENTINEL).all()), f"{what}: a neighbouring slice was written"


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("which", ["X", "dY"])
@pytest.mark.parametrize("M", [130, 128])
@pytest.mark.parametrize("N1,N2", list(WGRAD_TILES))
def test_wgrad_strided_operands_and_sliced_outputs_change_nothing(N1, N2, M, which, f16, accumulate):
    """X (the CLS rows: pitch 5 N2) or dY as a window of a NaN-filled [M + 3, 5 N] buffer; dW and dbias as the middle third of a fused gradient."""
    lib = ops._lib.load()
    assert wgrad_tile(lib, [(M, N1, N2)]) == WGRAD_TILES[(N1, N2)]
    dY, X, refW, refb = wgrad_problem(M, N1, N2, f16, 7)
    ws = torch.empty(ops.wgrad_workspace_elems(M, N1, N2), dtype=F32, device=DEV)
    control = wgrad_outputs(N1, N2, False)
    ops.wgrad(dY, X, control[1], M, ws, accumulate=accumulate, dbias=control[3])
    strided = wgrad_outputs(N1, N2, True)
    dYs = window(dY, M + 3, 5 * N1, 0) if which == "dY" else dY
    Xs = window(X, M + 3, 5 * N2, 0) if which == "X" else X
    ops.wgrad(dYs, Xs, strided[1], M, ws, accumulate=accumulate, dbias=strided[3])
    torch.cuda.synchronize()
    wgrad_check(control, strided, refW, refb, M, N1, accumulate, f"wgrad {M}x{N1}x{N2} strided {which}")


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M", [130, 128])
def test_wgrad_group_strided_operands_and_sliced_outputs_change_nothing(M, f16, accumulate):
    """The 256 x 256 tile exists for groups only: two (256, 256) problems through WgradQueue, one with strided X and one with strided dY."""
    N1 = N2 = 256
    lib = ops._lib.load()
    assert wgrad_tile(lib, [(M, N1, N2)] * 2) == (256, 256)
    probs = [wgrad_problem(M, N1, N2, f16, 11), wgrad_problem(M, N1, N2, f16, 12)]
    controls, strideds = [wgrad_outputs(N1, N2, False) for _ in probs], [wgrad_outputs(N1, N2, True) for _ in probs]
    q = ops.WgradQueue()
    for (dY, X, _, _), o in zip(probs, controls):
        q.add(dY, X, o[1], M, dbias=o[3])
    q.flush(accumulate=accumulate)
    for i, ((dY, X, _, _), o) in enumerate(zip(probs, strideds)):
        q.add(window(dY, M + 3, 5 * N1, 0) if i == 1 else dY, window(X, M + 3, 5 * N2, 0) if i == 0 else X, o[1], M, dbias=o[3])
    q.flush(accumulate=accumulate)
    torch.cuda.synchronize()
    for i, ((_, _, refW, refb), c, s) in enumerate(zip(probs, controls, strideds)):
        wgrad_check(c, s, refW, refb, M, N1, accumulate, f"wgrad_group problem {i} ({'strided X' if i == 0 else 'strided dY'})")
