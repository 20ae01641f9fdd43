"""The exactness proof of ``FlatIPIndex.search`` (csrc/topk.hip, above ``thresholds_kernel`` and ``select_compact_kernel``), checked link by link
on corpora built to spend the bound instead of 1-6 % of it:

  (1) ``eps[q] >= |fp16 scan score - exact centred score|`` for every row       - section b, through the production chain, every scan kernel;
  (2) the select keeps every candidate with scan score ``>= t^ - 2 eps``          - section c, against a numpy restatement;
  (3) the status bits are raised whenever that list is incomplete                - section c;
  and the three together on a corpus whose fp16 scan ranks 1024 wrong rows above the whole exact top-64 - section d.

The constructions and their restatements (``eps_ref``, ``max_norm_ref``, ``scan_emulated``, the corpus families, ``inversion_corpus``) live at
the top of this module and need numpy only; tests/test_search_proof_host.py holds them to their own claims without a GPU.

Every value of the symmetric corpora is a multiple of 2^-24 below 2^12 in magnitude and every row r comes with -r: at most 16 384 such values
sum EXACTLY in fp64 in any order (50 bits), so the column mean is 0 bit for bit on the host and on the device, and centring leaves the rows as
they were built."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops
from cldrd_amd.retriever import retrieval_utils as RU
from oracle import retrieval_ref as R
from test_gpu_retrieval import same_ranking
from test_gpu_index_fp16 import centred16, check_mu, oracle16

DEV = "cuda"
FAMILIES = ("aligned", "below_normal", "heavy_tailed", "common_component")
SYMMETRIC = ("aligned", "below_normal", "heavy_tailed")


# ---- restatements (numpy, fp64) ---------------------------------------------------------------------------------------------------
def eps_ref(qnorm, pmax, d):
    """``thresholds_kernel``'s bound, term by term: rounding of both operands, fp32 accumulation, values below the fp16 normal range.
    ``pmax`` crosses the C ABI as a float."""
    qn = np.atleast_1d(np.asarray(qnorm, dtype=np.float64))
    pm, dd = float(np.float32(pmax)), float(d)
    e = qn * pm * (2.0 ** -10 + 2.0 ** -22 + dd * 2.0 ** -22) + 2.0 ** -14 * math.sqrt(dd) * (qn + pm) + dd * 2.0 ** -28
    return (e * (1.0 + 1e-6)).astype(np.float32) + np.float32(1e-30)


def max_norm_ref(P, mu):
    """``FlatIPIndex._attach``: the largest centred row norm (fp32 subtraction, fp64 sum, held as fp32) plus 2^-12 of the largest raw one."""
    P, mu = np.asarray(P, dtype=np.float32), np.asarray(mu, dtype=np.float32)
    c = (P - mu).astype(np.float64)
    cnorm = math.sqrt(float(np.float32((c * c).sum(axis=1).max())))
    raw_max = math.sqrt(float(np.float32((P.astype(np.float64) ** 2).sum(axis=1).max())))
    return cnorm * (1.0 + 1e-6) + raw_max * 2.0 ** -12


def scan_emulated(q, P):
    """The scan as the bound models it: both operands rounded to fp16, products (exact in fp32: 11 + 11 bits) and the running sum in fp32,
    element order.  -> fp32 [nq, rows]"""
    q16 = np.atleast_2d(np.asarray(q, dtype=np.float32)).astype(np.float16).astype(np.float32)
    p16t = np.ascontiguousarray(np.asarray(P, dtype=np.float32).astype(np.float16).astype(np.float32).T)
    acc = np.zeros((q16.shape[0], p16t.shape[1]), dtype=np.float32)
    for j in range(p16t.shape[0]):
        acc += q16[:, j:j + 1] * p16t[j][None, :]
    return acc


# ---- corpus families ---------------------------------------------------------------------------------------------------------------
def _aligned(rng, shape, e, up=False):
    """(1 + (2k + 1) 2^-11)(1 -+ 2^-20) 2^e, k in 0..7: a hair below (``up``: above) the midpoint of two fp16 neighbours, so that fp16
    rounds EVERY element the same way by (almost) the full half ulp.  The fp32 value is 1 + (2k + 1) 2^-11 -+ 2^-20 exactly."""
    k = rng.integers(0, 8, size=shape)
    out = ((1.0 + (2 * k + 1) * 2.0 ** -11) * (1.0 + (2.0 ** -20 if up else -2.0 ** -20)) * np.exp2(e)).astype(np.float32)
    return out


def _grid24(x):
    """fp32 values as multiples of 2^-24 (those of magnitude >= 1/2 are already): see the module docstring."""
    x = np.asarray(x, dtype=np.float32).copy()
    small = np.abs(x) < 0.5
    x[small] = (np.rint(x[small].astype(np.float64) * 2.0 ** 24) * 2.0 ** -24).astype(np.float32)
    assert np.abs(x).max() < 4096.0
    return x


def _pairs(base):
    """rows r, -r interleaved: base row i is row 2 i"""
    out = np.empty((2 * base.shape[0], base.shape[1]), dtype=np.float32)
    out[0::2], out[1::2] = base, -base
    return out


@functools.lru_cache(maxsize=4)
def corpus(family, rows, d, nq=16):
    """(P fp32 [rows, d], Q fp32 [nq, d]) of one family; arrays are shared between tests: read-only."""
    half = rows // 2
    rng = np.random.default_rng([FAMILIES.index(family), rows, d])
    if family in ("aligned", "common_component"):
        # row i: exponent 3 - i % 7 (norms over seven binades), random signs.  Query j is base row 7 j - a row of the TOP binade, so that
        # |p| = pmax (within the spread of k) where q is parallel to p and every product q_j p_j is rounded down by 2^-10
        assert 7 * nq <= half
        e = (3 - np.arange(half) % 7)[:, None]
        base = _aligned(rng, (half, d), e) * rng.choice(np.float32([-1.0, 1.0]), size=(half, d))
        Q = base[0:7 * nq:7].copy()
        P = _pairs(base)
        if family == "common_component":
            m = rng.standard_normal(d)
            P = P + (m * (40.0 / np.linalg.norm(m))).astype(np.float32)          # fp32 addition: the rows lose their alignment by 2^-24 |p|
    elif family == "below_normal":
        P = _pairs(np.full((half, d), 0.9 * 2.0 ** -14, dtype=np.float32))
        Q = np.full((nq, d), 3.0, dtype=np.float32)
    elif family == "heavy_tailed":
        base = _grid24(rng.standard_normal((half, d)) * np.exp(1.5 * rng.standard_normal((half, 1))))
        P = _pairs(base)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
    else:
        raise ValueError(family)
    P.flags.writeable = Q.flags.writeable = False
    return P, Q


def host_premise(P, Q):
    """What the host can say about a corpus: mu (fp32 of the fp64 column mean), eps per query, and |scan_emulated - exact| / eps per pair,
    exact = <q, p - mu> in fp64 with the fp32 mu."""
    d = P.shape[1]
    mu = P.astype(np.float64).mean(axis=0).astype(np.float32)
    eps = eps_ref(np.linalg.norm(Q.astype(np.float64), axis=1).astype(np.float32), max_norm_ref(P, mu), d)
    exact = Q.astype(np.float64) @ (P.astype(np.float64) - mu.astype(np.float64)).T
    scan = scan_emulated(Q, P - mu)
    return mu, eps, np.abs(scan.astype(np.float64) - exact) / eps[:, None].astype(np.float64)


# ---- the inversion corpus ----------------------------------------------------------------------------------------------------------
N_A, N_B = 64, 1024


@functools.lru_cache(maxsize=2)
def inversion_corpus(d, n=16384):
    """One query and n > CAND_CAP rows on which the fp16 scan ranks 1024 rows (group B) above the whole exact top-64 (group A) by more than
    one eps - and, the bound being right, by less than two.

    Width = halves H1 | H2; the last four positions of each half are TRIM positions (fp16-representable in the query and in the rows: no
    rounding error there).  q is aligned-down on H1 and aligned-up on H2; A rows live on H1 (aligned-down), B rows on H2 (aligned-up): the
    scan scores A low by ~2^-10 <q, p> and B high by as much.  All at exponent 4 (elements ~16), where the bound's third term is < 1 % of
    the first.  The trim values bring, in fp64, every B score to one target T and A row i to T + (0.04 - 0.02 i / 63) eps: the exact top-64
    is A, row 0 of A first, least A - B gap 0.02 eps.  Then the negatives of all of these, and r, -r pairs of Gaussian rows of
    a tenth of A's norm up to n rows; everything permuted.  -> dict(P, q, A, B (row positions, A in rank order), eps)"""
    assert d % 8 == 0 and n % 2 == 0
    rng = np.random.default_rng([77, d])
    e, h = 4, d // 2
    body = h - 4
    qt = 2.0 ** e * np.array([1.0, 2.0 ** -4, 2.0 ** -8, 2.0 ** -11])
    q = np.zeros(d)
    q[:body], q[h:h + body] = _aligned(rng, body, e), _aligned(rng, body, e, up=True)
    q[body:h] = q[h + body:] = qt
    rows = np.zeros((N_A + N_B, d))
    rows[:N_A, :body] = _aligned(rng, (N_A, body), e)
    rows[N_A:, h:h + body] = _aligned(rng, (N_B, body), e, up=True)
    raw = rows @ q
    pmax0 = np.linalg.norm(rows, axis=1).max()
    eps0 = float(eps_ref(np.float32(np.linalg.norm(q)), pmax0 * (1.0 + 1e-6 + 2.0 ** -12), d)[0])
    target = np.full(N_A + N_B, raw.mean())
    target[:N_A] += (0.04 - 0.02 * np.arange(N_A) / (N_A - 1)) * eps0          # A row 0 ranks first
    for r in range(N_A + N_B):
        res, t0 = target[r] - raw[r], (body if r < N_A else h + body)
        for t in range(4):
            v = float(np.float16(res / qt[t]))
            if abs(v) < 2.0 ** -14:              # stay inside the fp16 normal range: a trim value must not depend on subnormal handling
                v = 0.0
            rows[r, t0 + t] = v
            res -= v * qt[t]
    sign = rng.choice([-1.0, 1.0], size=d)                                     # one sign per column, shared by q and the rows
    q, rows = q * sign, rows * sign
    n_fill = n // 2 - (N_A + N_B)
    fill = rng.standard_normal((n_fill, d))
    fill = _grid24(fill * (0.1 * pmax0 / np.linalg.norm(fill, axis=1, keepdims=True)))
    base = np.concatenate([rows, fill.astype(np.float64)])
    both = np.concatenate([base, -base])
    P = both.astype(np.float32)
    assert np.array_equal(P.astype(np.float64), both) and np.array_equal(q.astype(np.float32).astype(np.float64), q)      # all of it IS fp32
    perm = rng.permutation(n)
    P = np.ascontiguousarray(P[perm])
    pos = np.argsort(perm)
    q32 = q.astype(np.float32)
    eps = float(eps_ref(np.float32(np.linalg.norm(q)), max_norm_ref(P, np.zeros(d, dtype=np.float32)), d)[0])
    P.flags.writeable = q32.flags.writeable = False
    return dict(P=P, q=q32, A=pos[:N_A].copy(), B=pos[N_A:N_A + N_B].copy(), eps=eps)


def inversion_figures(inv, fp16_rows=False):
    """Exact scores (fp64; ``fp16_rows``: of the fp16-rounded rows, what that mode stores), emulated scan scores, and
    (least A - B gap of the exact scores, (min scan B - max scan A), (min err B - max err A)) in units of eps."""
    P, q, A, B, eps = inv["P"], inv["q"], inv["A"], inv["B"], inv["eps"]
    rows = P.astype(np.float16).astype(np.float64) if fp16_rows else P.astype(np.float64)
    exact = rows @ q.astype(np.float64)
    scan = scan_emulated(q, P)[0].astype(np.float64)
    err = scan - exact
    return exact, scan, ((exact[A].min() - exact[B].max()) / eps, (scan[B].min() - scan[A].max()) / eps, (err[B].min() - err[A].max()) / eps)


# ---- the table of measured ratios --------------------------------------------------------------------------------------------------
_RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    """The ratios section b measured go to the file CLDRD_PROOF_RATIOS_OUT names.  profiles/search_proof_ratios.txt is regenerated by
    ``CLDRD_PROOF_RATIOS_OUT=profiles/search_proof_ratios.txt python -m pytest -m gpu tests/test_gpu_search_proof.py`` on an MI355X; a plain
    run of the suite leaves the committed file alone and holds it to what it measures (``test_measured_ratios_agree_with_the_record``)."""
    yield
    path = os.environ.get("CLDRD_PROOF_RATIOS_OUT")
    if not path or not _RATIOS:
        return
    with open(path, "w") as fh:
        fh.write("max |fp16 scan score - exact centred score| / eps[q] over all (query, row) pairs, tests/test_gpu_search_proof.py section b\n")
        fh.write(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})\n")
        fh.write(f"{'family':<18}{'d':>6}{'rows':>7}{'nq':>5}  {'mode':<11}{'scan kernel':<26}{'ratio':>10}\n")
        for fam, d, rows, nq, mode, kern, ratio in _RATIOS:
            fh.write(f"{fam:<18}{d:>6}{rows:>7}{nq:>5}  {mode:<11}{kern:<26}{ratio:>10.4f}\n")
        bn = [r[-1] for r in _RATIOS if r[0] == "below_normal"]
        if bn:
            verdict = ("FLUSHED to zero (the emulation gives 0.90 then)" if min(bn) > 0.45 else
                       "KEPT (the emulation gives 0.0004 then)" if max(bn) < 0.05 else "handled differently from kernel to kernel")
            fh.write(f"below-normal family (row elements 0.9 * 2^-14, fp16-subnormal): ratios {min(bn):.4f} .. {max(bn):.4f}: the fp16 MFMA operands are {verdict}\n")


# ---- a. prep_queries and thresholds --------------------------------------------------------------------------------------------------
def _prep(q):
    nq, d = q.shape
    q32 = torch.from_numpy(np.array(q, dtype=np.float32, order="C")).to(DEV)          # a copy: the corpora's arrays are read-only
    qh = torch.empty(nq, d, dtype=torch.float16, device=DEV)
    qb = torch.empty(nq, d, dtype=torch.bfloat16, device=DEV)
    qnorm, flag = torch.empty(nq, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.topk_prep_queries(q32, qh, qb, qnorm, flag)
    return q32, qh, qb, qnorm, flag


@pytest.mark.parametrize("d", [128, 384, 768, 1024])
@pytest.mark.parametrize("nq", [1, 5, 130])
def test_prep_queries_and_thresholds_equal_their_restatements(nq, d):
    """qh / qb: torch's round-to-nearest-even casts, bit for bit (midpoints, fp16 subnormals, -0.0 and 65504 among the values).
    qnorm: the kernel sums d squares in fp32; ANY order of that sum is within d 2^-24 relative of the exact one (d - 1 additions and one
    product rounding per term), the square root halves it and rounds once more (2 ulp allowed for sqrtf): (d / 2 + 2) 2^-24 relative.
    eps: ``eps_ref`` of the kernel's OWN qnorm within 2 ulp (fp64 contraction, one fp32 rounding); thr = est - 2 eps exactly in fp32."""
    rng = np.random.default_rng([3, nq, d])
    q = (rng.standard_normal((nq, d)) * np.exp(rng.standard_normal((nq, 1)))).astype(np.float32)
    q[0, :8] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 65504.0, 1e-6, -3e-8, 2.0 ** -14 * 0.9, 1.0 + 2.0 ** -8]
    q32, qh, qb, qnorm, flag = _prep(q)
    assert int(flag.item()) == 0
    assert torch.equal(qh.view(torch.int16), q32.half().view(torch.int16))
    assert torch.equal(qb.view(torch.int16), q32.bfloat16().view(torch.int16))
    qn = qnorm.cpu().numpy()
    ref = np.linalg.norm(q.astype(np.float64), axis=1)
    rel = np.abs(qn.astype(np.float64) - ref) / ref
    print(f"prep nq={nq} d={d}: qnorm max rel err {rel.max():.2e} (bar {(d / 2 + 2) * 2.0 ** -24:.2e})")
    assert rel.max() <= (d / 2 + 2) * 2.0 ** -24
    pmax = 37.25 + 0.001 * d                       # not an fp32 value: the ABI rounds it
    est = torch.from_numpy((rng.standard_normal(nq) * 50.0).astype(np.float32)).to(DEV)
    thr, eps = torch.empty(nq, dtype=torch.float32, device=DEV), torch.empty(nq, dtype=torch.float32, device=DEV)
    ops.topk_thresholds(est, qnorm, pmax, d, thr, eps)
    eps_h, want = eps.cpu().numpy(), eps_ref(qn, pmax, d)
    ulps = np.abs(eps_h.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 2, (ulps.max(), eps_h[:4], want[:4])
    assert np.array_equal(thr.cpu().numpy(), est.cpu().numpy() - np.float32(2.0) * eps_h)
    eps2 = torch.empty(nq, dtype=torch.float32, device=DEV)
    ops.topk_thresholds(None, qnorm, pmax, d, None, eps2)                     # the exhaustive path's call: eps only
    assert torch.equal(eps, eps2)


@pytest.mark.parametrize("value,flagged", [(7e4, True), (float("inf"), True), (-float("inf"), True), (65504.0, False), (-65504.0, False)])
def test_range_flag_of_queries_and_index_rows(value, flagged):
    """|x| > 65504 or not finite does not fit the fp16 shadow: prep_queries raises its flag; index_center_cast does, and FlatIPIndex refuses
    the rows (both attach modes).  65504 itself fits.  The rows come in r, -r pairs (mu = 0), so the centred value IS the value."""
    d = 128
    q = np.random.default_rng(5).standard_normal((5, d)).astype(np.float32)
    q[3, 77] = value
    flag = _prep(q)[4]
    assert bool(flag.item()) == flagged
    base = _grid24(np.random.default_rng(6).standard_normal((40, d)))
    base[17, 5] = value
    P = _pairs(base)
    for fp16_rows in (False, True):
        index = RU.construct_flatindex_from_embeddings(P, None)
        if flagged:
            with pytest.raises(ValueError, match="65504"):
                RU.convert_index_to_gpu(index, 0, fp16_rows)
            with pytest.raises(RuntimeError, match="not on a GPU"):        # the refused shard is not searched
                index.search(q, 3)
        else:
            RU.convert_index_to_gpu(index, 0, fp16_rows)
            assert np.all(index.mu == 0) and float(index._p16[34, 5].item()) == value


# ---- b. the premise: eps >= |scan - exact| through the production chain --------------------------------------------------------------
def _scan_kernel(d, rows, nq, tiled):
    if not tiled and d in (128, 256, 768):
        return "stream 8x32 (256 queries)" if nq > 128 else "stream"
    return "ring-scan" if (rows >= 4096 and nq <= 128) else "128x128 filter"


def _scan_all(qh, p16, tiled):
    """scan scores fp32 [nq, rows] in row order: threshold -1e30, lists of `rows` slots - every pair is a hit, once"""
    nq, rows = qh.shape[0], p16.shape[0]
    thr = torch.full((nq,), -1e30, dtype=torch.float32, device=DEV)
    counts = torch.zeros(nq + 1, dtype=torch.int32, device=DEV)
    cr = torch.full((nq, rows), -1, dtype=torch.int32, device=DEV)
    cs = torch.zeros(nq, rows, dtype=torch.float32, device=DEV)
    ops.topk_scan_filter(qh, p16, thr, counts, cr, cs, tiled=tiled)
    c, crh, csh = counts.cpu().numpy(), cr.cpu().numpy().astype(np.int64), cs.cpu().numpy()
    assert np.all(c[:nq] == rows) and c[nq] == 0, (tiled, c[:4], c[nq])
    assert np.array_equal(np.sort(crh, axis=1), np.broadcast_to(np.arange(rows), (nq, rows)))       # every row once per query
    out = np.empty_like(csh)
    np.put_along_axis(out, crh, csh, axis=1)
    return out


def _premise_case(family, d, rows, fp16_rows, nq=16):
    P, Q = corpus(family, rows, d, nq)
    index = RU.construct_flatindex_from_embeddings(P, None)
    RU.convert_index_to_gpu(index, 0, fp16_rows)
    assert index.row_dtype == ("float16" if fp16_rows else "float32")
    mu = check_mu(index, P)                                        # within 1e-6 of max|mean|: exactly 0 on the symmetric families
    if family in SYMMETRIC:
        assert np.all(mu == 0)
    want_norm = max_norm_ref(P, mu)
    assert abs(index._max_norm - want_norm) <= 1e-6 * want_norm     # two fp32 roundings of squared norms (6e-8 each), the raw one times 2^-12
    q32, qh, qb, qnorm, flag = _prep(Q)
    assert int(flag.item()) == 0
    eps_d = torch.empty(nq, dtype=torch.float32, device=DEV)
    ops.topk_thresholds(None, qnorm, index._max_norm, d, None, eps_d)       # as search_device takes it
    eps = eps_d.cpu().numpy().astype(np.float64)
    r16 = index._p16.cpu().numpy()
    assert np.array_equal(r16.view(np.uint16), centred16(P, mu).view(np.uint16))
    q64 = Q.astype(np.float64)
    if fp16_rows:
        ref = q64 @ r16.astype(np.float64).T                         # the stored row IS mu + R16[r]; the scan scores its centred part
    else:
        ref = q64 @ (P.astype(np.float64) - mu.astype(np.float64)).T
    worst = {}
    for tiled in (False, True):
        if tiled and _scan_kernel(d, rows, min(nq, 128), True) == _scan_kernel(d, rows, nq, False):
            continue                                                 # no streaming kernel at this width: both entries take the same kernel
        if tiled and nq > 128:                                       # the tiled kernels take 128 queries per call (cldrd_flatip_search splits likewise)
            scan = np.concatenate([_scan_all(qh[lo:lo + 128].contiguous(), index._p16, True) for lo in range(0, nq, 128)])
        else:
            scan = _scan_all(qh, index._p16, tiled)
        ratio = np.abs(scan.astype(np.float64) - ref) / eps[:, None]
        kern = _scan_kernel(d, rows, min(nq, 128) if tiled else nq, tiled)
        worst[kern] = max(worst.get(kern, 0.0), float(ratio.max()))
        mode = "fp16 rows" if fp16_rows else "default"
        print(f"premise {family} d={d} rows={rows} nq={nq} {mode} {kern}: max |scan - exact| / eps = {ratio.max():.4f}")
        _RATIOS.append((family, d, rows, nq, mode, kern, float(ratio.max())))
        assert np.all(ratio <= 1.0), (family, d, rows, kern, float(ratio.max()))          # the proof's condition: no margin
        if family == "aligned" and d <= 768 and not fp16_rows:
            assert ratio.max() >= 0.5                               # the inputs reached the kernel as built (emulation: 0.83 - 0.94)
    return worst


@pytest.mark.parametrize("fp16_rows", [False, True], ids=["default", "fp16rows"])
@pytest.mark.parametrize("rows", [2048, 8192])
@pytest.mark.parametrize("d", [128, 768, 384, 1024])
@pytest.mark.parametrize("family", FAMILIES)
def test_eps_bounds_the_scan_error_on_adversarial_rounding(family, d, rows, fp16_rows):
    """|scan - exact| <= eps[q] for EVERY (query, row) pair, the scan once through cldrd_topk_scan_filter (streaming kernel at d = 128 / 768)
    and once through the tiled entry (ring-scan from 4096 rows, the 128 x 128 filter epilogue below), eps as search_device computes it.
    The reference is <q, p - mu> in fp64 with the index's own fp32 mu (fp16-row mode: <q, R16[r]>)."""
    _premise_case(family, d, rows, fp16_rows)


def test_eps_bounds_the_scan_error_in_the_256_query_form():
    """130 queries at d = 768: one pass of the two-batch streaming instance (8 waves x 32 queries)."""
    worst = _premise_case("aligned", 768, 2048, False, nq=130)
    assert "stream 8x32 (256 queries)" in worst


RATIOS_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "profiles", "search_proof_ratios.txt")


def _read_record(path):
    """{(family, d, rows, nq, mode, scan kernel): ratio} of the table ``_ratio_table`` wrote (fixed-width columns: kernel names hold blanks)"""
    rec = {}
    with open(path) as fh:
        for line in fh:
            if line[:18].strip() in FAMILIES:
                rec[(line[:18].strip(), int(line[18:24]), int(line[24:31]), int(line[31:36]), line[38:49].strip(), line[49:75].strip())] = float(line[75:85])
    return rec


def test_measured_ratios_agree_with_the_record():
    """profiles/search_proof_ratios.txt is a record of section b, and a record can go stale: every case measured in this run (the whole of
    section b in a run of the module; one case when this test runs alone) has its line there, within 0.02 of eps.  The corpora are seeded,
    so the same kernels reproduce their figures; a kernel that sums in another order moves a score by a few fp32 roundings, each
    2^-24 |score| <= 2^-14 eps, about sqrt(d) 2^-14 = 0.002 eps in all.  A change of the bound, of a corpus or of the handling of
    fp16 subnormals (0.0004 against 0.90) moves them by far more: regenerate the file then (``_ratio_table``) and look at what changed."""
    if os.environ.get("CLDRD_PROOF_RATIOS_OUT"):
        return                                                       # this run writes the record
    if not _RATIOS:
        _premise_case("aligned", 128, 2048, False)
    rec = _read_record(RATIOS_RECORD)
    for fam, d, rows, nq, mode, kern, ratio in _RATIOS:
        key = (fam, d, rows, nq, mode, kern)
        assert key in rec, f"{key} is not in profiles/search_proof_ratios.txt"
        assert abs(ratio - rec[key]) <= 0.02, (key, ratio, rec[key])


# ---- c. the select ------------------------------------------------------------------------------------------------------------------
def _ord(x):
    """the kernel's monotone float -> uint32 map (-0.0 sorts below +0.0)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint32)


def _unord(o):
    o = np.asarray(o, dtype=np.uint32).astype(np.uint64)
    return np.where(o & 0x80000000, o & 0x7FFFFFFF, ~o & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def _cut(khat, eps):
    """the next float below float32(float64(khat) - 2 float64(eps))"""
    x = np.float32(np.float64(khat) - 2.0 * np.float64(eps))
    return _unord(np.uint32(int(_ord(x)) - 1))[()]


def select_ref(c, dropped, rows, scores, cap, kk, thr, eps, cap2, exhaustive):
    """One query of select_compact_kernel by definition -> (status, khat, kept row set).  With fewer than kk valid entries there is no khat
    (-inf), no cut and no bit 8: everything is kept and bit 1 or 2 says why the list proves nothing."""
    n = min(c, cap)
    s, r = scores[:n], rows[:n]
    st, khat, cut = 0, np.float32(-np.inf), np.float32(-np.inf)
    if not exhaustive:
        st |= (1 if c < kk else 0) | (2 if c > cap else 0) | (4 if dropped != 0 else 0)
        if n >= kk:
            khat = _unord(np.sort(_ord(s))[n - kk])[()]
            cut = _cut(khat, eps)
            if not thr <= cut:
                st |= 8
    kept = set(r[s >= cut].tolist())
    if len(kept) > cap2:
        st |= 16
    return st, khat, kept, cut


def _select_lists(cap, kk, cap2, rng):
    """12 candidate lists (count, scores of the min(count, cap) valid entries, eps, thr or a function of the cut) - see the test.
    Degenerate parametrizations: with cap = 100 < kk = 1000 no list has kk valid entries (no khat, no cut, no bit 8: bits 1 / 2 only, everything
    kept); the 'cap2 + 1' list can exceed cap2 only when cap > cap2, i.e. at cap = 8192, cap2 = 1024 (bit 16 is raised there alone); the test's
    sanity asserts on the named cases run where cap >= kk + 40."""
    big = min(cap, kk + 40)
    L = []
    s = (rng.standard_normal(big) * 10).astype(np.float32)                    # 0: ties at khat
    if big > kk:
        o = np.argsort(-s)
        s[o[max(0, kk - 3):kk + 2]] = s[o[kk - 1]]
    L.append((big, s, 0.01, -1e30))
    n1 = min(cap, 2 * kk + 20)                                                # 1: both signs, +0.0 and -0.0 around khat
    s = np.concatenate([np.abs(rng.standard_normal(max(0, min(kk - 1, n1 - 8)))) + 0.5, [0.0, -0.0, -0.0, 0.0, -0.001, -0.0015, -0.0025, -0.5],
                        -np.abs(rng.standard_normal(n1)) - 1.0])[:n1].astype(np.float32)
    L.append((n1, rng.permutation(s), 1e-3, -1e30))
    x = np.float32(3e4)                                                       # 2: khat = 3e4, eps = 1e-3: fp32(khat - 2 eps) rounds UP to khat - 1 ulp
    below = [np.nextafter(x, np.float32(0))]
    for _ in range(3):
        below.append(np.nextafter(below[-1], np.float32(0)))                  # khat - 1, 2, 3, 4 ulp: the first two are kept
    top = x + np.arange(min(kk, max(cap - 6, 1)), dtype=np.float32) * np.float32(2.0 ** -8)
    s = np.concatenate([top, below, [100.0, -3e4]]).astype(np.float32)[:cap]
    L.append((len(s), rng.permutation(s), 1e-3, -1e30))
    for c in (kk, kk - 1, 0):                                                 # 3, 4, 5: c == kk, kk - 1, 0
        L.append((c, (rng.standard_normal(min(c, cap)) * 3).astype(np.float32), 0.05, -1e30))
    L.append((cap + 5, (rng.standard_normal(cap) * 5).astype(np.float32), 0.02, -1e30))          # 6: overflow, only cap entries exist
    s = (rng.standard_normal(big) * 7 + 20).astype(np.float32)
    L.append((big, s, 0.03, "cut"))                                           # 7: thr == cut
    L.append((big, s.copy(), 0.03, "above"))                                  # 8: thr = the float after cut
    n9 = min(cap, cap2 + 21)                                                  # 9: cap2 + 1 rows in the band (where the list can hold them)
    s = np.concatenate([np.full(min(n9, cap2 + 1), 5.0) + rng.integers(0, 3, min(n9, cap2 + 1)) * 1e-4, np.full(max(0, n9 - cap2 - 1), -7.0)]).astype(np.float32)
    L.append((n9, rng.permutation(s), 1e-3, -1e30))
    s = (rng.standard_normal(cap) * 100).astype(np.float32)                   # 10: a full list, a wide band
    L.append((cap, s, 15.0, -1e30))
    n11 = max(1, cap // 3)                                                    # 11: all negative, large magnitudes
    L.append((n11, (-np.abs(rng.standard_normal(n11)) * 1e6 - 1.0).astype(np.float32), 2e3, -1e30))
    return L


@pytest.mark.parametrize("cap2", [1024, 8192])
@pytest.mark.parametrize("kk", [1, 10, 1000])
@pytest.mark.parametrize("cap", [100, 8192])
def test_select_keeps_the_two_eps_band_and_raises_the_status_bits(cap, kk, cap2):
    """cldrd_topk_select on 12 hand-built lists in one launch, then the same lists with a dropped-hit count (bit 4 everywhere) and with
    exhaustive = True (keep all, status 0).  Expected, by definition: khat = kk-th largest score; cut = the next float below
    fp32(khat - 2 eps); kept = exactly the rows with score >= cut; n2 = min(|kept|, cap2); bits 1: c < kk, 2: c > cap, 4: dropped,
    8: not thr <= cut, 16: |kept| > cap2.  Slots past a list's end hold 1e30 scores: reading them would show."""
    rng = np.random.default_rng([9, cap, kk, cap2])
    lists = _select_lists(cap, kk, cap2, rng)
    nq = len(lists)
    assert nq == 12
    counts = np.zeros(nq + 1, dtype=np.int32)
    rows = np.full((nq, cap), -7, dtype=np.int32)
    scores = np.full((nq, cap), 1e30, dtype=np.float32)
    eps = np.zeros(nq, dtype=np.float32)
    thr = np.zeros(nq, dtype=np.float32)
    for i, (c, s, e, t) in enumerate(lists):
        n = min(c, cap)
        assert len(s) == n
        counts[i], eps[i] = c, e
        scores[i, :n] = s
        rows[i, :n] = rng.permutation(1 << 20)[:n]
        if isinstance(t, str) and n < kk:
            t = -1e30                                                 # a list too short to have a khat has no cut either
        elif isinstance(t, str):
            cut = _cut(_unord(np.sort(_ord(s))[n - kk])[()], eps[i])
            t = cut if t == "cut" else np.nextafter(cut, np.float32(np.inf))
        thr[i] = t
    if cap >= kk + 40:      # the cases are what their names say (where the list is long enough to have a khat)
        k0 = np.sort(scores[0, :counts[0]])[::-1][kk - 1]
        assert (scores[0, :counts[0]] == k0).sum() >= 2
        assert np.sort(scores[2, :counts[2]])[::-1][kk - 1] == np.float32(3e4)
        assert np.float32(np.float64(3e4) - 2.0 * np.float64(eps[2])) == np.nextafter(np.float32(3e4), np.float32(0))         # rounded up, to khat - 1 ulp
    for dropped, exhaustive in ((0, False), (3, False), (0, True)):
        counts[nq] = dropped
        d_counts, d_rows, d_scores = (torch.from_numpy(a).to(DEV) for a in (counts, rows, scores))
        rows2 = torch.full((nq, cap2), -1, dtype=torch.int32, device=DEV)
        n2, status = torch.full((nq,), -5, dtype=torch.int32, device=DEV), torch.full((nq,), -5, dtype=torch.int32, device=DEV)
        khat = torch.full((nq,), 123.0, dtype=torch.float32, device=DEV)
        ops.topk_select(d_counts, d_rows, d_scores, kk, torch.from_numpy(thr).to(DEV), torch.from_numpy(eps).to(DEV), rows2, n2, status, khat,
                        exhaustive=exhaustive)
        r2, n2h, sth, kh = rows2.cpu().numpy(), n2.cpu().numpy(), status.cpu().numpy(), khat.cpu().numpy()
        seen = 0
        for i in range(nq):
            st, k_ref, kept, cut = select_ref(int(counts[i]), dropped, rows[i], scores[i], cap, kk, thr[i], eps[i], cap2, exhaustive)
            tag = (cap, kk, cap2, dropped, exhaustive, i)
            assert sth[i] == st, (tag, sth[i], st)
            assert kh[i] == k_ref, (tag, kh[i], k_ref)
            assert n2h[i] == min(len(kept), cap2), (tag, n2h[i], len(kept))
            got = r2[i, :n2h[i]].tolist()
            assert len(set(got)) == len(got) and np.all(r2[i, n2h[i]:] == -1), tag
            if len(kept) <= cap2:
                assert set(got) == kept, (tag, sorted(set(got) ^ kept)[:8], cut)
            else:
                assert set(got) <= kept, tag                          # any cap2 of them
            seen |= st
        if not exhaustive and not dropped and cap == 8192 and kk <= 10 and cap2 == 1024:
            assert seen == (1 | 2 | 8 | 16)                            # every bit the lists can raise was raised by one of them
        if exhaustive:
            assert np.all(sth[n2h < cap2] == 0) and np.all(np.isneginf(kh))


# ---- d. the inversion corpus end to end -----------------------------------------------------------------------------------------------
INVERSION_WIDTHS = (128, 768)


def _attach_inversion(d, fp16_rows, **hooks):
    inv = inversion_corpus(d)
    P = inv["P"]
    ids = np.arange(P.shape[0], dtype=np.int64) * 3 + 5
    index = RU.construct_flatindex_from_embeddings(P, ids)
    index.profile = True                                          # last_stats counts the emitted and the re-scored rows
    for k_, v_ in hooks.items():
        setattr(index, k_, v_)
    RU.convert_index_to_gpu(index, 0, fp16_rows)
    assert np.all(check_mu(index, P) == 0)
    return inv, ids, index


@functools.lru_cache(maxsize=4)
def _inversion_oracle(d, fp16_rows):
    inv = inversion_corpus(d)
    P, q = inv["P"], inv["q"][None, :]
    ids = np.arange(P.shape[0], dtype=np.int64) * 3 + 5
    if fp16_rows:
        return oracle16(np.zeros(d, dtype=np.float32), P.astype(np.float16), q, N_A, ids=ids)
    return R.flat_ip_search(P, ids, q, N_A)


@pytest.mark.parametrize("variant", ["default", "query_tile_128", "repeated"])
@pytest.mark.parametrize("d", INVERSION_WIDTHS)
def test_search_returns_the_exact_top64_where_the_scan_inverts_it(d, variant):
    """The fp16 scan puts all 1024 B rows above every A row, by more than eps (tests/test_search_proof_host.py); the exact top-64 is A.  The
    search must return A, in the oracle's order with the oracle's scores, PROVEN (not exhaustive, no exact fallback) - as one query, with
    128-query tiles, and repeated so often that the search runs a probe pass and a rest."""
    inv, ids, index = _attach_inversion(d, False, **({"query_tile_request": 128} if variant == "query_tile_128" else {}))
    # "repeated": a search probes only when it has more than two query tiles.  300 queries at 128-query tiles (d = 128); at d = 768 the
    # default tile is 256 and 300 queries would be two plain passes, so the count follows the tile: 556
    reps = 1 if variant != "repeated" else 2 * index.query_tile + 44
    q = np.repeat(inv["q"][None, :], reps, axis=0)
    D, I = index.search(q, N_A)
    st = index.last_stats
    print(f"inversion d={d} {variant}: {reps} queries, scan emitted {st['candidates']} rows, re-scored {st['rescored']} in the first pass; "
          f"scans {st['scans']}, rescans {st['rescans']}, first-pass status bits {st['status_bits_first_pass']}")
    Dr, Ir = _inversion_oracle(d, False)
    assert np.array_equal(Ir[0], ids[inv["A"]])                   # the oracle agrees with the construction: A, row 0 of A first
    Dr, Ir = np.repeat(Dr, reps, axis=0), np.repeat(Ir, reps, axis=0)
    assert np.array_equal(I, Ir)
    same_ranking(D, I, Dr, Ir)
    assert np.array_equal(D, Dr)
    assert st["exhaustive"] is False and st["fallback_queries"] == 0, st
    if variant == "repeated":
        assert "cap2" in st and st["scans"] >= 3                  # probe pass + rest
    if variant == "query_tile_128":
        assert index.query_tile == 128


@pytest.mark.parametrize("d", INVERSION_WIDTHS)
def test_inversion_corpus_in_fp16_row_mode_equals_its_oracle(d):
    """fp16-row mode stores the rounded rows: only q rounds in the scan (about 0.6 eps between the groups), and the exact top-64 of THOSE
    rows is what ``oracle16`` says (B rows: their stored values were rounded up)."""
    inv, ids, index = _attach_inversion(d, True)
    D, I = index.search(inv["q"][None, :], N_A)
    st = index.last_stats
    print(f"inversion d={d} fp16 rows: scan emitted {st['candidates']} rows, re-scored {st['rescored']} in the first pass; scans {st['scans']}, "
          f"rescans {st['rescans']}, first-pass status bits {st['status_bits_first_pass']}")
    Dr, Ir = _inversion_oracle(d, True)
    same_ranking(D, I, Dr, Ir)
    assert np.array_equal(D, Dr)
    assert st["exhaustive"] is False and st["fallback_queries"] == 0, st


# ---- e. non-streaming widths above CAND_CAP ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16_rows", [False, True], ids=["default", "fp16rows"])
@pytest.mark.parametrize("d", [384, 1024])
def test_search_at_widths_without_a_streaming_kernel(d, fp16_rows):
    """d = 384 / 1024 (BERT-large) above CAND_CAP rows: scan through the ring-scan and the filter epilogue, select, proof - against the
    oracle of the mode, with an exact duplicate row and a query that is a corpus row."""
    n, nq = 20000, 150
    emb = syn.corpus_embeddings(111, n, d)
    emb[n // 2] = emb[n // 3]
    q = syn.corpus_embeddings(112, nq, d)
    q[0] = emb[17] * 1.0
    ids = np.arange(n, dtype=np.int64) * 3 + 5
    index = RU.construct_flatindex_from_embeddings(emb, ids)
    RU.convert_index_to_gpu(index, 0, fp16_rows)
    mu = check_mu(index, emb)
    r16 = centred16(emb, mu) if fp16_rows else None
    for k in (10, 1000):
        D, I = index.search(q, k)
        st = index.last_stats
        Dr, Ir = oracle16(mu, r16, q, k, ids=ids) if fp16_rows else R.flat_ip_search(emb, ids, q, k)
        same_ranking(D, I, Dr, Ir)
        assert np.all(np.diff(D, axis=1) <= 0)
        assert st["exhaustive"] is False and st["fallback_queries"] == 0, st
    assert I[0, 0] == ids[17]
