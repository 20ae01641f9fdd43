"""The deterministic mode of the embedding backward (--deterministic) on the GPU: the inverted index (key_order), the fixed-order per-key
sums (segment_sum_rows), the rows form of the embedding backward, run-to-run equality, and the training step - two runs equal, graph replay
equal to the eager step, the default (atomic) path equal outside the tables.

C = hip_ops.SEGMENT_CHUNK.  The summation order the references below spell out is the one of include/cldrd_hip.h: a key's rows in ascending
row order, cut into chunks of C entries, each chunk summed left to right, the chunk sums added left to right."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cldrd_amd.synthetic as syn
from cldrd_amd import hip_ops as ops
from cldrd_amd.encoder import EncoderConfig
from cldrd_amd.models import NwayDualEncoder
from cldrd_amd.trainer import NwayTrainer
from oracle import dropout_ref as DR

DEV = "cuda"
C = ops.SEGMENT_CHUNK


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy((syn.normal(seed, int(np.prod(shape))) * scale).astype(np.float32).reshape(shape))


# ------------------------------------------------------------------------------------------------ key_order
def _check_order(keys, n_keys):
    order, offsets = ops.key_order(torch.from_numpy(keys).to(DEV), n_keys)
    assert order.dtype == torch.int32 and offsets.dtype == torch.int32
    kc = np.clip(keys, 0, n_keys - 1)
    want = np.argsort(kc, kind="stable").astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(np.bincount(kc, minlength=n_keys))]).astype(np.int32)
    assert torch.equal(order.cpu(), torch.from_numpy(want))
    assert torch.equal(offsets.cpu(), torch.from_numpy(starts))


@pytest.mark.parametrize("n_keys", [1, 7, 30522])
@pytest.mark.parametrize("T", [1, 63, 64, 257, 4099])
def test_key_order_is_the_stable_argsort(T, n_keys):
    _check_order(syn.randint(1000 + T + n_keys, 0, n_keys, T), n_keys)                    # uniform keys
    _check_order(np.full(T, n_keys // 2, dtype=np.int64), n_keys)                         # all keys equal
    ends = np.where(syn.randint(7 + T, 0, 2, T) == 0, 0, n_keys - 1).astype(np.int64)     # only the first and the last key populated
    _check_order(ends, n_keys)
    _check_order(syn.randint(2000 + T + n_keys, -5, n_keys + 5, T), n_keys)               # out of range: clamped like the ids
    if n_keys > 256:
        # heavy duplicates next to singletons, keys that differ in the high digit only
        hot = np.where(syn.randint(9 + T, 0, 3, T) == 0, syn.randint(11 + T, 0, n_keys, T), (syn.randint(13 + T, 0, 4, T) * 256 + 101))
        _check_order(hot.astype(np.int64), n_keys)


# ------------------------------------------------------------------------------------------------ segment_sum_rows
def _wide_rows(seed, T, d):
    """fp32 rows whose magnitudes span 2^-10 .. 2^10: the order of the adds shows in the low bits"""
    e = syn.randint(seed + 1, -10, 11, T * d).reshape(T, d).astype(np.float64)
    return (syn.normal(seed, T * d).reshape(T, d) * np.exp2(e)).astype(np.float32)


def _segment_ref(rows, lists, out0, accumulate):
    """numpy float32, exactly the order of include/cldrd_hip.h; lists: {key: ascending row numbers}"""
    out = out0.copy()
    for k, lst in lists.items():
        s = None
        for c0 in range(0, len(lst), C):
            cs = rows[lst[c0]].copy()
            for r in lst[c0 + 1:c0 + C]:
                cs = cs + rows[r]
            s = cs if s is None else s + cs
        out[k] = out0[k] + s if accumulate else s
    assert out.dtype == np.float32
    return out


def _lists_of(keys, n_keys):
    return {k: np.nonzero(keys == k)[0] for k in range(n_keys) if (keys == k).any()}


def _run_segment(rows, keys, n_keys, accumulate, strided=False):
    T, d = rows.shape
    out0 = rnd(5, (n_keys, d)).numpy() * 3.0 + 7.0                        # the sentinel empty keys must keep
    out = torch.from_numpy(out0).to(DEV)
    if strided:
        ops.segment_sum_rows(torch.from_numpy(rows).to(DEV), None, None, out, accumulate=accumulate)
    else:
        order = torch.from_numpy(np.argsort(keys, kind="stable").astype(np.int32)).to(DEV)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_keys))]).astype(np.int32)).to(DEV)
        ops.segment_sum_rows(torch.from_numpy(rows).to(DEV), order, offsets, out, accumulate=accumulate)
    want = _segment_ref(rows, _lists_of(keys, n_keys), out0, accumulate)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    return out


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("d", [4, 128, 768, 1024])
def test_segment_sum_rows_follows_the_documented_order(d, accumulate):
    # list lengths 1, C-1, C, C+1, 2C, 3C+7 on keys spread over several workgroups of 16 keys, empty keys between them
    lens = {0: 1, 5: C - 1, 63: C, 64: C + 1, 100: 2 * C, 139: 3 * C + 7}
    n_keys = 140
    keys = np.concatenate([np.full(n, k, dtype=np.int64) for k, n in lens.items()])
    keys = keys[np.argsort(syn.uniform01(31, keys.size), kind="stable")]          # rows of a key scattered over the input
    rows = _wide_rows(40 + d, keys.size, d)
    _run_segment(rows, keys, n_keys, accumulate)
    # the adds are not associative on this input: the plain left-to-right sum of the longest list differs from the chunked one
    lst = np.nonzero(keys == 139)[0]
    plain = rows[lst[0]].copy()
    for r in lst[1:]:
        plain = plain + rows[r]
    chunked = _segment_ref(rows, {139: lst}, np.zeros((n_keys, d), np.float32), False)[139]
    assert d < 128 or not np.array_equal(plain, chunked)
    # one key holds every row (the shape rule then gives the key a whole workgroup)
    T1 = 2 * C + 5
    _run_segment(_wide_rows(50 + d, T1, d), np.zeros(T1, dtype=np.int64), 1, accumulate)
    # the strided form: row r has key r % n_keys, T no multiple of n_keys; long lists (a workgroup per key) and short ones (16 keys per workgroup)
    for n_k, T in ((5, 5 * (C + 3) + 2), (40, 103)):
        _run_segment(_wide_rows(60 + d + n_k, T, d), np.arange(T, dtype=np.int64) % n_k, n_k, accumulate, strided=True)


# ------------------------------------------------------------------------------------------------ embed_ln_bwd_rows / embed_ln_bwd_det
VARIANTS = {
    # name: (dy format, dy_branch format, dropout, packed positions, loss scale S)
    "bf16": (torch.bfloat16, None, 0.0, False, None),
    "f32+branch,dropout": (torch.float32, torch.bfloat16, 0.1, False, None),
    "f32,packed": (torch.float32, None, 0.0, True, None),
    "f16+branch,dropout,packed,scaled": (torch.float16, torch.float16, 0.1, True, 4.0),
}


def _embed_case(V, P, d, M, L, variant):
    """One embedding block: inputs on the device, the float64 autograd gradients, and a closure that runs a backward form."""
    fmt, bfmt, p, packed, S = VARIANTS[variant]
    seed = 1234567
    if packed:
        lens = 1 + syn.randint(70, 0, L, M)
        lens[0] = L
        pos_np = np.concatenate([np.arange(n) for n in lens]).astype(np.int64)
    else:
        pos_np = np.arange(M * L, dtype=np.int64) % L
    T = pos_np.size
    word, pos, typ = rnd(20, (V, d)), rnd(21, (P, d)), rnd(22, (2, d))
    gamma, beta = 1 + rnd(23, (d,), 0.1), rnd(24, (d,), 0.1)
    ids_np = syn.randint(25, 0, V, T)
    ids_np[::3] = ids_np[0]                                   # a hot token: a third of the rows
    ids = torch.from_numpy(ids_np)
    dy = rnd(26, (T, d)).to(torch.bfloat16).float()           # representable in every stream format
    dy[5] = 0.0                                               # a row without gradient (a padded position)
    # float64 reference (tests/test_gpu_kernels.py: test_embed_ln_fwd_bwd), the dropout mask from the numpy mirror of the kernels' hash
    w, p_, t_ = (a.double().requires_grad_(True) for a in (word, pos, typ))
    g_, b_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(w[ids] + p_[torch.from_numpy(pos_np)] + t_[0], (d,), g_, b_, 1e-12)
    if p > 0:
        y = y * torch.from_numpy(DR.keep_mask(seed, p, T, d)).double() / (1.0 - p)
    y.backward(dy.double())
    ref = dict(dword=w.grad, dpos=p_.grad, dtype0=t_.grad[0], dgamma=g_.grad, dbeta=b_.grad)
    wd, pd, td, gd, bd = (a.to(DEV) for a in (word, pos, typ, gamma, beta))
    ids_d = ids.to(DEV)
    pos_idx = torch.from_numpy(pos_np.astype(np.int32)).to(DEV) if packed else None
    out = torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    ops.embed_ln_fwd(ids_d, wd, pd, td[0], gd, bd, out, mean, rstd, T, L, 1e-12, p, seed, pos_idx=pos_idx)
    scale = S if S is not None else 1.0
    if bfmt is None:
        dy_d, br_d = (dy * scale).to(fmt).to(DEV), None
    else:
        half = (dy * 0.5).to(torch.bfloat16).float()          # stream + branch add up to dy
        dy_d, br_d = ((dy - half) * scale).to(fmt).to(DEV), (half * scale).to(bfmt).to(DEV)
    state = None
    if S is not None:
        state = ops.new_loss_scale_state(DEV)
        state[0], state[1] = S, 1.0 / S
    partial = torch.empty(ops.ln_partial_elems(T, d), device=DEV)

    def run(form, word_t, pos_t, ids_t, pidx, dword, dpos, **kw):
        dtyp, dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
        with ops.loss_scale(state.data_ptr() if state is not None else None):
            form(dy_d, ids_t, word_t, pos_t, td[0], gd, mean, rstd, dword, dpos, dtyp, dg, db, partial, T, L, p, seed, accumulate=False,
                 pos_idx=pidx, dy_branch=br_d, **kw)
        return dtyp, dg, db

    return dict(T=T, d=d, L=L, V=V, P=P, ids=ids_d, pos_np=pos_np, pos_idx=pos_idx, word=wd, pos=pd, ref=ref, run=run)


def _close(got, ref, name):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs()
    tol = 1e-3 * ref.abs().max().item() + 1e-3 * ref.abs()
    assert int((err > tol).sum()) == 0, f"{name}: max err {err.max().item():.4e} (ref max {ref.abs().max().item():.3e})"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("V,P,d,M,L", [(300, 40, 256, 6, 20), (500, 64, 1024, 3, 50)])
def test_embed_ln_bwd_rows_and_det(V, P, d, M, L, variant):
    c = _embed_case(V, P, d, M, L, variant)
    T = c["T"]
    # per-row reference from the EXISTING atomic op on the expanded problem: token r owns row r of both tables, so each row is added once onto zero
    word_x = c["word"][c["ids"]].contiguous()
    pos_x = c["pos"][torch.from_numpy(c["pos_np"]).to(DEV)].contiguous()
    ar64, ar32 = torch.arange(T, device=DEV), torch.arange(T, device=DEV, dtype=torch.int32)
    dword_x, dpos_x = torch.zeros(T, d, device=DEV), torch.zeros(T, d, device=DEV)
    c["run"](ops.embed_ln_bwd, word_x, pos_x, ar64, ar32, dword_x, dpos_x)
    assert torch.equal(dword_x, dpos_x)
    rows = torch.full((ops.pad_rows(T), d), float("nan"), device=DEV)

    def rows_form(dy, ids, word, pos, type0, gamma, mean, rstd, dword, dpos, *a, **kw):
        return ops.embed_ln_bwd_rows(dy, ids, word, pos, type0, gamma, mean, rstd, rows, *a, **kw)
    dtyp_r, dg_r, db_r = c["run"](rows_form, c["word"], c["pos"], c["ids"], c["pos_idx"], None, None)
    assert not torch.isnan(rows[:T]).any()                    # every row written
    assert float(rows[5].abs().max()) == 0.0                  # zeros for the row without gradient
    err = (rows[:T] - dword_x).abs().max().item()
    print(f"embed_ln_bwd_rows ({variant}, d = {d}): max |rows - atomic per-row reference| = {err:.3e}, bit-identical: {torch.equal(rows[:T], dword_x)}")
    assert err <= 1e-6 * dword_x.abs().max().item()
    # the whole deterministic backward against the float64 autograd reference, and its LayerNorm gradients against the atomic form's bits
    word_order = ops.key_order(c["ids"], V)
    pos_order = ops.key_order(c["pos_idx"].to(torch.int64), L) if c["pos_idx"] is not None else None
    dword, dpos = torch.zeros(V, d, device=DEV), torch.zeros(P, d, device=DEV)
    dtyp, dg, db = c["run"](ops.embed_ln_bwd_det, c["word"], c["pos"], c["ids"], c["pos_idx"], dword, dpos, word_order=word_order,
                            pos_order=pos_order, rows=torch.empty(ops.pad_rows(T), d, device=DEV))
    for got, name in ((dword, "dword"), (dpos, "dpos"), (dtyp, "dtype0"), (dg, "dgamma"), (db, "dbeta")):
        _close(got, c["ref"][name], f"{variant}: {name}")
    dword_a, dpos_a = torch.zeros(V, d, device=DEV), torch.zeros(P, d, device=DEV)
    dtyp_a, dg_a, db_a = c["run"](ops.embed_ln_bwd, c["word"], c["pos"], c["ids"], c["pos_idx"], dword_a, dpos_a)
    for a, b, r in ((dtyp_a, dtyp, dtyp_r), (dg_a, dg, dg_r), (db_a, db, db_r)):
        assert torch.equal(a, b) and torch.equal(a, r)        # same grid, same partials: the bits of the atomic form
    assert (dword - dword_a).abs().max().item() <= 1e-5 * max(1.0, dword_a.abs().max().item())
    # accumulate: a second backward adds onto the first (two tapes of a shared tower)
    c["run"](ops.embed_ln_bwd_det, c["word"], c["pos"], c["ids"], c["pos_idx"], dword, dpos, word_order=word_order, pos_order=pos_order,
             rows=torch.empty(ops.pad_rows(T), d, device=DEV))
    _close(dword, 2 * c["ref"]["dword"], f"{variant}: dword twice")
    _close(dpos, 2 * c["ref"]["dpos"], f"{variant}: dpos twice")


def test_five_runs_of_the_deterministic_backward_give_the_same_bits():
    V, P, d, L = 64, 64, 768, 64
    T = 4099
    M = (T + L - 1) // L
    word, pos = rnd(80, (V, d)).to(DEV), rnd(81, (P, d)).to(DEV)
    gamma, beta = (1 + rnd(82, (d,), 0.1)).to(DEV), rnd(83, (d,), 0.1).to(DEV)
    ids_np = syn.randint(84, 0, V, T)
    ids_np[::2] = 0                                           # [PAD]-like: half the rows on one key
    ids = torch.from_numpy(ids_np).to(DEV)
    dy = rnd(85, (T, d)).to(torch.bfloat16).to(DEV)
    out = torch.empty(T, d, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    ops.embed_ln_fwd(ids, word, pos, None, gamma, beta, out, mean, rstd, T, L, 1e-12, 0.1, 99)
    partial = torch.empty(ops.ln_partial_elems(T, d), device=DEV)
    first = None
    for run in range(5):
        word_order = ops.key_order(ids, V)
        dword, dpos = torch.zeros(V, d, device=DEV), torch.zeros(P, d, device=DEV)
        dg, db = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
        ops.embed_ln_bwd_det(dy, ids, word, pos, None, gamma, mean, rstd, dword, dpos, None, dg, db, partial, T, L, 0.1, 99, accumulate=False,
                             word_order=word_order, pos_order=None, rows=torch.empty(ops.pad_rows(T), d, device=DEV))
        got = [t.clone() for t in (dword, dpos, dg, db, word_order[0], word_order[1])]
        if first is None:
            first = got
            assert float(dword.abs().max()) > 0 and float(dpos.abs().max()) > 0
        else:
            for a, b in zip(first, got):
                assert torch.equal(a, b), run


# ------------------------------------------------------------------------------------------------ the training step
def small_cfg(arch="distilbert", layers=2):          # the tiny config of tests/test_gpu_model.py, dropout on
    return EncoderConfig(arch=arch, vocab_size=512, dim=128, n_heads=2, hidden_dim=256, n_layers=layers,
                         max_position_embeddings=64, dropout=0.1, attention_dropout=0.1)


def _trainer(share, deterministic=True, **kw):
    cfg = small_cfg()
    torch.manual_seed(0)
    model = NwayDualEncoder(cfg, share_weights=share).cuda().train()
    with torch.no_grad():
        for seed, tower in zip((11, 12), model.towers()):
            for name, p in tower.named_flat():
                p.copy_(syn.init_param(seed, name, tuple(p.shape), std=0.05, perturb=True))
    return cfg, model, NwayTrainer(model, loss="kl_div", learning_rate=3e-3, warmup_steps=5, total_steps=40, deterministic=deterministic, **kw)


def _ragged(cfg, seed, B, N, Lq, Lp, packed, distill=False):
    """a batch with passage lengths spread over 2 .. Lp (tests/test_gpu_model.py: _ragged_batch); ``packed``: with the host lengths"""
    batch = syn.nway_batch(seed, B, N, Lq, Lp, vocab=cfg.vocab_size, ragged=True, label_kind="teacher", with_teacher_scores=distill)
    lens = 2 + syn.randint(seed + 77, 0, Lp - 1, B * N).astype(np.int64)
    mask = (np.arange(Lp)[None, :] < lens[:, None]).astype(np.int64)
    ids = np.where(mask == 1, batch["nway_passages"]["input_ids"].reshape(B * N, Lp).numpy(), 0)
    ids[np.arange(B * N), lens - 1] = 2
    batch["nway_passages"] = {"input_ids": torch.from_numpy(ids).view(B, N, Lp), "attention_mask": torch.from_numpy(mask).view(B, N, Lp)}
    out = {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in batch.items()}
    if packed:
        out["nway_passages"]["lengths"] = torch.from_numpy(lens)
    return out


@pytest.mark.parametrize("share,packed,amp,extra", [
    (False, False, "fp16", None), (False, True, "fp16", None), (True, False, "fp16", None), (True, True, "fp16", None),
    (False, False, "bf16", None), (False, True, "bf16", None), (True, False, "bf16", None), (True, True, "bf16", None),
    (False, False, "fp16", "zero_all_grads"), (False, False, "fp16", "distill"), (False, True, "fp16", "distill")])
def test_two_deterministic_runs_end_in_the_same_bits(share, packed, amp, extra, monkeypatch):
    """Two trainers from the same seeds, eight steps on the same ragged batches (unshared padded runs replay the step as a HIP graph from the
    fourth step on): parameters and both Adam moments bit for bit, embedding tables included."""
    monkeypatch.setenv("CLDRD_AMP", amp)
    ends = []
    for run in range(2):
        cfg, model, tr = _trainer(share, distill="kl_div" if extra == "distill" else None)
        tr.zero_all_grads = extra == "zero_all_grads"
        assert all(t.deterministic_embed for t in model.towers())
        for i in range(8):
            tr.train_step(_ragged(cfg, 300 + i, 3, 4, 8, 16, packed, distill=extra == "distill"))
        torch.cuda.synchronize()
        ends.append((tr.flat_p.clone(), tr.m.clone(), tr.v.clone()))
        assert torch.isfinite(tr.flat_p).all().item()
        off, shape = model.towers()[-1].layout.entries["embeddings.word_embeddings.weight"]
        toff = model._tower_offsets[-1]
        assert float(tr.m[toff + off:toff + off + shape[0] * shape[1]].abs().max()) > 0          # the word table did receive gradients
    for a, b, name in zip(ends[0], ends[1], ("flat_p", "m", "v")):
        assert torch.equal(a, b), name


def test_deterministic_graph_replay_equals_the_eager_step_bit_for_bit(monkeypatch):
    """The protocol of tests/test_gpu_model.py: test_graph_replay_of_the_training_step_equals_the_eager_step with the mode on: from identical
    state the replayed step and the plain eager step agree in loss, logits, the WHOLE gradient buffer and the updated parameters - no mask over
    the embedding tables, no rounding bar.  The orders are rebuilt inside the replay from that step's ids: the batches change every step."""
    monkeypatch.setenv("CLDRD_GRAPH", "1")
    cfg, model, tr = _trainer(False)
    towers = model.towers()

    def snapshot():
        return (tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.global_step, tr.adam_step, [t.step_seed for t in towers])

    def restore(sn):
        tr.flat_p.copy_(sn[0]); tr.m.copy_(sn[1]); tr.v.copy_(sn[2])
        tr.global_step, tr.adam_step = sn[3], sn[4]
        for t, ss in zip(towers, sn[5]):
            t.step_seed = ss
            t.refresh_shadows(need_transposed=True)

    replays = 0
    for i in range(11):
        shape = (3, 4, 8, 16) if i != 8 else (2, 3, 8, 16)
        batch = _ragged(cfg, 100 + i, *shape, packed=False)
        sn = snapshot()
        monkeypatch.setenv("CLDRD_GRAPH", "1")
        l1 = tr.train_step(batch).clone()
        lg1, g1, p1 = tr.last_logits.clone(), tr.flat_g.clone(), tr.flat_p.clone()
        key = tr._batch_key(batch)
        replayed = key in getattr(tr, "_graphs", {}) and tr._graphs[key]["graph"] is not None
        replays += int(replayed)
        restore(sn)                                   # the plain eager step from the same state: no device-side step state at all
        state, ptrs = tr._state, [getattr(t, "seed_base_ptr", None) for t in towers]
        tr._state = None
        for t in towers:
            t.seed_base_ptr = None
        monkeypatch.setenv("CLDRD_GRAPH", "0")
        l0 = tr.train_step(batch).clone()
        tr._state = state
        for t, pp in zip(towers, ptrs):
            t.seed_base_ptr = pp
        torch.cuda.synchronize()
        assert torch.equal(l1, l0), (i, replayed, l1, l0)
        assert torch.equal(lg1, tr.last_logits), (i, replayed)
        assert torch.equal(g1, tr.flat_g), (i, replayed)
        assert torch.equal(p1, tr.flat_p), (i, replayed)
    assert replays >= 6, replays
    assert tr.global_step == tr.adam_step == 11


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_deterministic_gradients_against_the_default_path(share, packed, monkeypatch):
    """From the same state and seeds: everything outside the embedding tables bit for bit what the default (atomic) path writes; the tables within
    the project's bar for atomic-order differences, 1e-5 * max(1, max|g|) (tests/test_gpu_model.py)."""
    monkeypatch.setenv("CLDRD_GRAPH", "0")
    cfg, model, tr = _trainer(share)
    towers = model.towers()
    emb = torch.zeros(tr.flat_p.numel(), dtype=torch.bool, device="cuda")
    for t, toff in zip(towers, model._tower_offsets):
        for n in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight"):
            off, shape = t.layout.entries[n]
            emb[toff + off:toff + off + shape[0] * shape[1]] = True
    batch = _ragged(cfg, 500, 3, 4, 8, 16, packed)
    seeds = [t.step_seed for t in towers]
    got = {}
    for det in (True, False):
        for t, ss in zip(towers, seeds):
            t.step_seed, t.deterministic_embed = ss, det
        loss, logits = tr.forward_backward(batch)
        torch.cuda.synchronize()
        got[det] = (loss.clone(), logits.clone(), tr.flat_g.clone())
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    g1, g0 = got[True][2], got[False][2]
    assert torch.equal(g1[~emb], g0[~emb])
    assert float(g1[emb].abs().max()) > 0
    ge = (g1[emb] - g0[emb]).abs().max().item()
    print(f"deterministic vs atomic tables (share {share}, packed {packed}): max |diff| {ge:.3e}, max |g| {g0[emb].abs().max().item():.3e}")
    assert ge <= 1e-5 * max(1.0, g0[emb].abs().max().item())
