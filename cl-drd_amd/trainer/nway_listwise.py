"""Training step of the multistep-curriculum trainers (reference ``trainer/multistep-curriculum/nway_listwise_{1,2,3}.py``,
step loop ``nway_listwise_1.py:328-367``), MI355X-native and data-parallel over RCCL.

One process per GPU (``torch.distributed`` backend "nccl" == RCCL over xGMI).  Per step, on each rank:

    forward (query tower, passage tower) -> scoring -> loss value + dlogits (one kernel) -> hand-written backward
    -> per-layer gradient buckets all-reduced on a side stream while the backward of earlier layers still runs
    -> clip_grad_norm_(max_grad_norm): its sums of squares taken in two pieces under the backward on one GPU (`_ClipNormPlan`), one pass otherwise
    -> legacy-HF AdamW, which also writes the 16-bit weight shadows the next step reads (fp16 in the default mode, where no training pass
    reads the bf16 one and it is left stale; bf16 under ``CLDRD_AMP=bf16``) -> linear schedule

Differences from the reference, on purpose (SURVEY.md sections 7, 8a14):
  * mixed precision is hand-placed instead of autocast: every MFMA operand of a training pass is fp16 (the reference's own
    ``use_fp16`` mode, loss-scaled backward); ``CLDRD_AMP=bf16`` is the all-bf16 mode - every operand of the forward, the tape and the
    backward bf16, no loss scale; fp32 accumulate, residual stream, gradient stream and master weights in both;
  * the loss scale is a power of two recomputed from dL/dCLS every step (``cldrd_loss_scale_adapt``), where ``GradScaler`` starts at
    65 536 and searches by overflowing: no early skipped steps here; what is kept is the safety net (a non-finite gradient norm skips the
    step, which - as in ``scaler.step`` - does not advance Adam's bias-correction step);
  * no per-step D2H sync: loss / train-MRR are read back only every ``logging_steps``;
  * the three stage scripts differ only in defaults, so there is one trainer with a ``--loss`` selector
    (default ``lambda_mrr`` as in the reference);
  * ``--distill_loss kl_div | margin_mse`` adds ``distill_alpha * kd(logits[:, :nway], batch["teacher_scores"])`` to that loss (one more
    launch on the loss stream, ``cldrd_distill_term``): the role of the knowledge-distillation trainers the reference's scripts name
    (``scripts/unity/kd_nway_listwise.sh``, ``logit_reg_nway_listwise.sh``) but never published;
  * ``--loss lambda_loss`` trains on allRank's LambdaLoss (``losses/standard_lambda_rank.py:3-117``; ``--weighing_scheme`` and the
    ``--lambda_*`` flags are its arguments) in the same place on the loss stream, one launch (``cldrd_lambda_term``); with
    ``--label_source teacher`` its labels are ``batch["teacher_scores"]`` instead of the label-mode constants (``--neg_score_mode``,
    ``--teacher_label_shift``): the role of the ``ndcg_nway_listwise*`` trainers the reference's scripts name but its tree lacks, so what
    these two flags mean is defined here (README: nDCG training);
  * ``--loss softmax_ce`` trains on the softmax cross-entropy (InfoNCE) of a row's positives against its negatives at ``--ce_temperature``,
    the loss the in-batch columns of ``--in_batch_loss`` and cosine scoring are normally paired with (``cldrd_softmax_ce``, one launch in the
    same place on the loss stream; ``--ce_pos_min`` / ``--ce_neg_max`` say which labels are positives and negatives, ``--ce_mask_duplicate_pids``
    keeps a passage that is a row's positive or neutral out of its negatives): the reference has no such loss, the definition is this
    package's (README: Contrastive training);
  * ``--apply_consine_similarity`` (the reference's spelling, ``scripts/unity/cosine_nway_listwise.sh``; its trainer is not in the tree)
    scores with ``--cosine_scale`` times the cosine of the two CLS embeddings instead of their dot product (``cldrd_score_cos_fwd`` /
    ``cldrd_score_cos_bwd`` in the place of the dot-product pair on the loss stream, one launch more); the checkpoint then carries a
    ``score`` key, which index, retrieval and validation read (README: Cosine-similarity scoring);
  * ``--dev_path / --dev_queries_path / --dev_qrels_path`` (the reference's flags): at every saved checkpoint rank 0 re-ranks the dev run with
    the student (``NwayTrainer.validate``: evaluation.DevPool + RerankingEvaluator) and writes ``dev_logs.log`` / ``dev_best.json``; the
    reference tokenises and encodes every (query, passage) pair of the run per validation, here each distinct text once;
  * ``--resume CKPT --resume_exact`` goes on where the checkpoint was written instead of restarting its epoch (``--resume`` alone: the
    reference's behaviour, unchanged): checkpoints carry one more key, ``resume_state`` - dropout step counters, the loss-scale block, both
    step counts (`NwayTrainer.resume_state`) and the data position (`train`, `_EpochPosition`) - and are moved into place whole
    (`save_checkpoint`).  With ``--deterministic`` the resumed run equals the uninterrupted one bit for bit (one process).
"""
from __future__ import annotations

import copy
import math
import os
import sys

import torch
import torch.distributed as dist

from .. import hip_ops as ops
from ..dataset.nway_dataset import attach_lengths
from ..encoder import HD32_EVAL_ONLY, _env_flag
from ..models.nway_dual_encoder import NwayDualEncoder, _lengths, score_mode
from ..retriever.retrieval_utils import cap_host_threads

LOSS_KINDS = ("lambda_mrr", "ranknet", "kl_div", "margin_mse", "lambda_loss")
DISTILL_KINDS = ("kl_div", "margin_mse")      # --distill_loss: the term on batch["teacher_scores"] added to the rank loss
# --loss softmax_ce (cldrd_softmax_ce in the fused step; this package's definition, README: Contrastive training), in a tuple of its own:
# --loss takes LOSS_KINDS + CONTRASTIVE_KINDS.  CE_DEFAULTS: the options that mean something under it only (ce_pos_min None: the row's
# maximum label is its positive), None = not set on the command line and in NwayTrainer; --ce_mask_duplicate_pids is a switch.
CONTRASTIVE_KINDS = ("softmax_ce",)
CE_DEFAULTS = {"ce_temperature": 1.0, "ce_pos_min": None, "ce_neg_max": 0.0}
# --loss lambda_loss (allRank's LambdaLoss framework, reference losses/standard_lambda_rank.py:3-117; cldrd_lambda_term in the fused step).
# The reference's launch scripts name ndcg trainers (--weighing_scheme, --neg_score_mode) that its tree does not contain: which labels the
# loss sees (LABEL_SOURCES) and what the two teacher-label options do are THIS package's definition (README: nDCG training).
WEIGHING_SCHEMES = tuple(k_ for k_ in ops.LAMBDA_SCHEMES if k_ is not None) + ("none",)       # --weighing_scheme; none: every pair weighs 1
LABEL_SOURCES = ("rank", "teacher")           # --label_source: the label-mode constants | batch["teacher_scores"] as the labels
NEG_SCORE_MODES = ("original", "mean")        # --neg_score_mode: the teacher's score of every negative | their mean for all of them
LABEL_SHIFTS = ("none", "row_min")            # --teacher_label_shift: row_min subtracts the row's lowest score (lambda_loss clamps labels at 0)
# the options that mean something under --loss lambda_loss only, with the reference function's defaults (lambda_k 0: no truncation)
LAMBDA_DEFAULTS = {"weighing_scheme": "none", "lambda_k": 0, "lambda_sigma": 1.0, "lambda_mu": 10.0, "lambda_gain": "power",
                   "lambda_log": "natural"}
TEACHER_LABEL_DEFAULTS = {"neg_score_mode": "original", "teacher_label_shift": "none"}
RESUME_VERSION = 1                            # of the checkpoint's "resume_state" (NwayTrainer.resume_state, train())
# what the data position of a checkpoint depends on: an exact resume under another value of any of them is refused (check_resume_position)
POSITION_FIELDS = ("train_batch_size", "nranks", "seed", "dataset_len", "steps_per_epoch", "num_train_epochs")
# two more under --tas_clusters (the file as given and a digest of its bytes): present in a checkpoint only when the run had the flag
TAS_POSITION_FIELDS = ("tas_clusters", "tas_clusters_digest")


def check_loss_options(loss, label_source="rank", in_batch_loss=False, label_mode=None, synthetic=False, given=(), *, ce_temperature=None,
                       ce_pos_min=None, ce_neg_max=None, ce_mask_duplicate_pids=False):
    """The combinations of --loss / --label_source / the lambda flags / the ce flags that mean nothing: a ``ValueError`` that names the flag.
    ``given``: the names of LAMBDA_DEFAULTS / TEACHER_LABEL_DEFAULTS set by the caller (None = not set, on the command line and in
    NwayTrainer); the ce flags come as their values (None / False = not set)."""
    if label_source not in LABEL_SOURCES:
        raise ValueError(f"--label_source must be one of {LABEL_SOURCES}")
    for name in given:
        if name in LAMBDA_DEFAULTS and loss != "lambda_loss":
            raise ValueError(f"--{name} is an option of --loss lambda_loss; it was given with --loss {loss}")
        if name in TEACHER_LABEL_DEFAULTS and label_source != "teacher":
            raise ValueError(f"--{name} is an option of --label_source teacher; it was given with --label_source {label_source}")
    if label_source == "teacher":
        if loss != "lambda_loss":
            raise ValueError(f"--label_source teacher needs --loss lambda_loss (the other rank losses read the label-mode constants); got --loss {loss}")
        if in_batch_loss:
            raise ValueError("--label_source teacher cannot go with --in_batch_loss: the in-batch columns have no teacher score")
        if label_mode == "1" and not synthetic:
            raise ValueError("--label_source teacher needs a relT / most-hard / semi-hard training file with scores; --label_mode 1 files have none")
    ce = {"ce_temperature": ce_temperature, "ce_pos_min": ce_pos_min, "ce_neg_max": ce_neg_max, "ce_mask_duplicate_pids": ce_mask_duplicate_pids or None}
    if loss not in CONTRASTIVE_KINDS:
        for name, value in ce.items():
            if value is not None:
                raise ValueError(f"--{name} is an option of --loss softmax_ce; it was given with --loss {loss}")
        return
    if ce_temperature is not None and not (math.isfinite(ce_temperature) and ce_temperature > 0.0):
        raise ValueError("--ce_temperature must be finite and > 0")
    neg_max = CE_DEFAULTS["ce_neg_max"] if ce_neg_max is None else float(ce_neg_max)
    if not math.isfinite(neg_max):
        raise ValueError("--ce_neg_max must be finite")
    if ce_pos_min is not None and not float(ce_pos_min) > neg_max:
        raise ValueError(f"--ce_pos_min must be > --ce_neg_max ({neg_max}): a label cannot make its column a positive and a negative")
    if label_mode is not None and not synthetic and not in_batch_loss:
        # the label row is a constant of the label mode: a row without a negative column of its own is never valid without in-batch columns
        from ..dataset.nway_dataset import _REL, labels_for_mode
        if str(label_mode) in _REL:
            row = labels_for_mode(str(label_mode))
            pos = [(v >= ce_pos_min) if ce_pos_min is not None else (v == max(row)) for v in row]
            if not any(v <= neg_max and not p_ for v, p_ in zip(row, pos)):
                raise ValueError(f"--label_mode {label_mode} has no negative column under --loss softmax_ce (no label <= --ce_neg_max {neg_max}): "
                                 "it needs the in-batch columns of --in_batch_loss")


def no_decay(name: str) -> bool:
    """reference nway_listwise_1.py:259-263 (substring match on 'bias' / 'LayerNorm.weight')."""
    return ("bias" in name) or ("LayerNorm.weight" in name)


def linear_schedule_factor(step: int, warmup_steps: int, total_steps: int) -> float:
    """``transformers.get_linear_schedule_with_warmup`` lambda (reference nway_listwise_1.py:265)."""
    if step < warmup_steps:
        return float(step) / float(max(1, warmup_steps))
    return max(0.0, float(total_steps - step) / float(max(1, total_steps - warmup_steps)))


def allreduce_buckets(flat_g: torch.Tensor, buckets, world: int, group=None):
    """SUM all-reduce of every (tower, layer, start, end) bucket of the flat gradient buffer (blocking form; the trainer
    issues the same calls per bucket from the backward hooks on a side stream).  The division by world_size is folded
    into dlogits, so the reduced buffer already holds the mean gradient."""
    if world <= 1:
        return
    for _, _, a, b in buckets:
        dist.all_reduce(flat_g[a:b], op=dist.ReduceOp.SUM, group=group)


def owns_example(line_idx: int, rank: int, nranks: int) -> bool:
    """Data sharding rule of the reference (dataset/nway_dataset.py:305): example line i belongs to rank i % nranks."""
    return line_idx % nranks == rank


def optimizer_param_groups(model):
    """Parameter names in the reference optimizer's index order: ``model.named_parameters()`` of the (DDP-wrapped)
    NwayDualEncoder - HF module order, a shared tower listed once under ``query_encoder`` - split into the decayed group, then
    the no-decay group (nway_listwise_1.py:259-263); torch numbers the parameters consecutively over the groups.
    Returns [[(full name, tower index or None for parameters this package does not hold (BERT pooler), HF name)]] per group."""
    from ..encoder import hf_parameter_order
    names = []
    for ti, (prefix, tower) in enumerate((("query_encoder", model.query_encoder), ("passage_encoder", model.passage_encoder))):
        if ti == 1 and model.share_weights:
            break
        for n in hf_parameter_order(tower.cfg, with_pooler=True):
            names.append((f"{prefix}.{n}", ti if n in tower.layout.entries else None, n))
    return [[e for e in names if not no_decay(e[0])], [e for e in names if no_decay(e[0])]]


class _ClipNormPlan:
    """The sums of squares behind ``clip_grad_norm_``: the partial-sum buffer and what one step decides about it.

    One GPU: the norm is taken in two pieces.  When the passage tower's embedding block is complete (hook -1, called BEFORE its last
    weight-gradient group is launched) every gradient of the query tower (whose backward is already queued on the second stream) and of that
    block is final: [0, split) of the joint buffer, two thirds of it.  Their sums of squares are taken on the second stream UNDER the 3-ms
    weight-gradient launch (HBM reads next to an MFMA-bound kernel); after it only the passage tower's layers are left (`launch`).  Same fp64
    reduction of fp32 partial sums as the one-piece norm.

    ``partial``: [0, half) the early piece (sqnorm_partial on the second stream), [half, 2 half) the late piece when it is taken by
    sqnorm_partial, or [half, half + used) when the kernels that write the passage tower's layer gradients leave them (norm sink, round 5).
    Sink capacity from the layout: a weight-gradient group's slab reduction takes <= 256 slots per problem (4 per layer + the CLS-only
    layer's split projections), a LayerNorm-parameter reduction ceil(3 d / 64) per LayerNorm (2 per layer + embeddings): 12-layer towers
    (cfg4) need 13.4 k slots - a fixed 12 288 silently sent them back to the separate norm pass."""

    def __init__(self, model, flat_g):
        self.flat_g, self.tower = flat_g, model.passage_encoder       # the tower that is handed the sink and reports the slots it used
        pt = model.towers()[-1]
        self.early_end = model._tower_offsets[-1] + pt.layout.embed_range[1]          # where the early piece ends when there is one
        self.half = ops.sqnorm_blocks() // 2
        self.sink_cap = 256 * (4 * pt.cfg.n_layers + 4) + ((3 * pt.cfg.dim + 63) // 64) * (2 * pt.cfg.n_layers + 2)
        self.partial = torch.empty(self.half + self.sink_cap, dtype=torch.float32, device=flat_g.device)
        self.sink = self.partial[self.half:self.half + self.sink_cap]
        self.warned = False                # the "sink too small" warning is given once per trainer
        self.begin_step()

    def begin_step(self):
        """A backward starts (or a capture was abandoned): one-piece norm and no sink until this step says otherwise."""
        self.split = None                  # the early piece covers flat_g[:split]
        self.deferred = None               # (event on the main stream, second stream) of an early piece that is still to be enqueued
        self.sink_on = False
        self.tower.norm_sink, self.tower.norm_sink_used = None, -1

    def early_hook(self, main, side, defer, use_sink):
        """This step takes the norm in two pieces: -> the passage tower's ``after_layer`` hook; the tower is handed the sink if ``use_sink``."""
        self.sink_on = bool(use_sink)
        if use_sink:
            self.tower.norm_sink = self.sink

        def hook(layer):
            if layer != -1 or self.early_end % 4 != 0 or self.early_end >= self.flat_g.numel():
                return
            ev = torch.cuda.Event()
            ev.record(main)
            self.deferred = (ev, side)
            # defer: the query tower's backward is enqueued BEHIND the passage tower's (graph capture, see _backward): the partial norm has to
            # follow it on the second stream - `_backward` calls enqueue_early then - and still only waits for THIS point of the main stream
            if not defer:
                self.enqueue_early()
        return hook

    def enqueue_early(self):
        if self.deferred is None:
            return
        (ev, side), self.deferred = self.deferred, None
        side.wait_event(ev)
        with torch.cuda.stream(side):
            ops.sqnorm_partial(self.flat_g[:self.early_end], self.partial, self.half)
        self.split = self.early_end

    def launch(self, flat_g, max_norm, clip_out):
        """The rest of the norm and the clip coefficient, on the current stream (which has joined the second one since the early piece)."""
        split, half = self.split, self.half
        if not split:
            ops.grad_clip_coef(flat_g, max_norm, self.partial, clip_out)
            return
        # [0, split) was summed on the second stream during the backward.  The rest - the passage tower's layer gradients - is final only
        # behind its last weight-gradient group; when that group's slab reduction and the LayerNorm-parameter reduction left their sums of
        # squares (norm sink), nothing is re-read; else one more pass over them
        used = int(self.tower.norm_sink_used)
        if self.sink_on and used > 0:
            ops.clip_coef(self.partial, half + used, max_norm, clip_out)
            return
        if self.sink_on and used == -2 and not self.warned:
            self.warned = True
            import warnings
            warnings.warn(f"clip norm: the norm sink ({self.sink_cap} slots) is too small for this tower's gradient launches; "
                          "taking the late piece with a separate pass")
        ops.sqnorm_partial(flat_g[split:], self.partial[half:2 * half], half)
        ops.clip_coef(self.partial, 2 * half, max_norm, clip_out)


class _CapturePolicy:
    """Which steps are captured into a HIP graph and which are replayed: counts and batch keys only, nothing of torch.

    ``decide(key, eligible)`` is asked once per train_step that wants a graph at all (``eligible``: the batch is padded - a packed batch
    changes its row count every step) and answers EAGER, VOTE_NO (eager, after a "no" in the ranks' agreement), CAPTURE (capture, then replay)
    or REPLAY; ``record(key, ok)`` takes the agreed outcome of a CAPTURE or VOTE_NO.

    One GPU: a shape runs eager for its first ``warm`` eligible calls (allocator warm-up, one-time kernel attributes), is captured on the
    next and replayed from then on; ``max_shapes`` shapes at most are followed (the last partial batch is dropped, drop_last: a few shapes)
    - a shape first seen when that many are known stays eager for good; one failed capture leaves everything eager for good.

    Data parallel: ranks that replay captured collectives must all do so for the SAME steps, or the collectives of one rank's replay meet
    another rank's eager launches in another order / never (a hang no capture-time check can see).  So: (a) the decision is taken ONCE, at
    call number ``warm`` + 1 on every rank - the count advances for EVERY call, eligible or not (whether a rank's batch is packed depends on
    its own token fill: a count of eligible calls would reach the agreement at different global steps on different ranks, or never, and the
    one-off all-reduce would meet another rank's bucket all-reduces); there a rank captures its batch shape if it is eligible and the only
    one seen so far, ``warm`` times, else it votes "no"; one all_reduce(MIN) of the outcomes: a single failure anywhere leaves every rank
    eager for good; (b) afterwards only that ONE shape replays - an eager step of another shape issues the same bucket all-reduces in the
    same order as a replay does, so mixing the two across ranks is safe; a second capture (another agreement collective at a rank-dependent
    step) would not be."""
    EAGER, VOTE_NO, CAPTURE, REPLAY = "eager", "vote-no", "capture", "replay"

    def __init__(self, warm, ddp, max_shapes=4):
        self.warm, self.ddp, self.max_shapes = warm, ddp, max_shapes
        self.calls = 0              # decide() calls under ``ddp``
        self.seen = {}              # batch key -> eligible eager calls so far
        self.captured = set()
        self.broken = False

    def decide(self, key, eligible):
        if self.broken:
            return self.EAGER
        vote = False
        if self.ddp:
            self.calls += 1
            vote = self.calls == self.warm + 1
        if not eligible:
            return self.VOTE_NO if vote else self.EAGER
        if key in self.captured:
            return self.REPLAY
        if (self.ddp and self.calls > self.warm + 1) or (key not in self.seen and len(self.seen) >= self.max_shapes):
            return self.EAGER
        n = self.seen.setdefault(key, 0)
        if vote:
            return self.CAPTURE if (len(self.seen) == 1 and n >= self.warm) else self.VOTE_NO
        if n < self.warm or self.ddp:
            self.seen[key] = n + 1
            return self.EAGER
        return self.CAPTURE

    def record(self, key, ok):
        if ok:
            self.captured.add(key)
        else:
            self.broken = True


class NwayTrainer:
    def __init__(self, model: NwayDualEncoder, *, loss: str = "lambda_mrr", T: float = 1.0, learning_rate: float = 7e-6,
                 weight_decay: float = 0.01, adam_epsilon: float = 1e-8, max_grad_norm: float = 1.0, warmup_steps: int = 4000,
                 total_steps: int = 100000, betas=(0.9, 0.999), bucket_layers: int = 1, reg_lambda: float = 0.0,
                 distill=None, distill_alpha: float = 1.0, distill_T: float = 1.0, distill_only: bool = False,
                 deterministic: bool = False, weighing_scheme=None, lambda_k=None, lambda_sigma=None, lambda_mu=None, lambda_gain=None,
                 lambda_log=None, label_source: str = "rank", neg_score_mode=None, teacher_label_shift=None, n_rel=None, ce_temperature=None,
                 ce_pos_min=None, ce_neg_max=None, ce_mask_duplicate_pids: bool = False):
        if loss not in LOSS_KINDS + CONTRASTIVE_KINDS:
            raise ValueError(f"loss must be one of {LOSS_KINDS + CONTRASTIVE_KINDS}")
        opts = dict(weighing_scheme=weighing_scheme, lambda_k=lambda_k, lambda_sigma=lambda_sigma, lambda_mu=lambda_mu, lambda_gain=lambda_gain,
                    lambda_log=lambda_log, neg_score_mode=neg_score_mode, teacher_label_shift=teacher_label_shift)
        check_loss_options(loss, label_source, getattr(model, "in_batch_loss", False), given=[k_ for k_, v_ in opts.items() if v_ is not None],
                           ce_temperature=ce_temperature, ce_pos_min=ce_pos_min, ce_neg_max=ce_neg_max, ce_mask_duplicate_pids=ce_mask_duplicate_pids)
        opts = {k_: ({**LAMBDA_DEFAULTS, **TEACHER_LABEL_DEFAULTS}[k_] if v_ is None else v_) for k_, v_ in opts.items()}
        for name, allowed in (("weighing_scheme", WEIGHING_SCHEMES), ("lambda_gain", ("power", "linear")), ("lambda_log", ("natural", "binary")),
                              ("neg_score_mode", NEG_SCORE_MODES), ("teacher_label_shift", LABEL_SHIFTS)):
            if opts[name] not in allowed:
                raise ValueError(f"--{name} must be one of {allowed}")
        if int(opts["lambda_k"]) < 0 or not float(opts["lambda_sigma"]) > 0.0:
            raise ValueError("--lambda_k must be >= 0 (0: no truncation) and --lambda_sigma > 0")
        if opts["neg_score_mode"] == "mean" and n_rel is None:
            raise ValueError("--neg_score_mode mean needs n_rel, the number of relT passages of the label mode")
        # --loss lambda_loss: the keyword arguments of ops.lambda_term.  label_source "teacher": the slate is the row's own nway columns, its
        # labels this step's teacher scores (transformed inside the kernel: they stay the one per-step input of a captured step), no padding
        self.label_source = label_source
        self._lambda_kw = dict(weighing_scheme=None if opts["weighing_scheme"] == "none" else opts["weighing_scheme"],
                               k=int(opts["lambda_k"]) or None, sigma=float(opts["lambda_sigma"]), mu=float(opts["lambda_mu"]),
                               gain=opts["lambda_gain"], reduction_log=opts["lambda_log"])
        if label_source == "teacher":
            self._lambda_kw.update(padded_value_indicator=float("-inf"), neg_mean=opts["neg_score_mode"] == "mean",
                                   row_min=opts["teacher_label_shift"] == "row_min", n_rel=n_rel)
        # --loss softmax_ce: the keyword arguments of ops.softmax_ce; with ce_mask_duplicate_pids this step's batch["nway_pids"] go with them
        self._ce_kw = dict(temperature=float(CE_DEFAULTS["ce_temperature"] if ce_temperature is None else ce_temperature),
                           pos_min=None if ce_pos_min is None else float(ce_pos_min),
                           neg_max=float(CE_DEFAULTS["ce_neg_max"] if ce_neg_max is None else ce_neg_max))
        self.ce_mask_duplicate_pids = bool(ce_mask_duplicate_pids)
        if distill is not None and distill not in DISTILL_KINDS:
            raise ValueError(f"distill must be None or one of {DISTILL_KINDS}")
        if distill is not None and (not float(distill_alpha) >= 0.0 or not float(distill_T) > 0.0):
            raise ValueError("distill_alpha must be >= 0 and distill_T > 0")
        if distill_only and distill is None:
            raise ValueError("distill_only needs a distill loss")
        if any(t.cfg.head_dim == 32 for t in model.towers()):
            raise ValueError("NwayTrainer: " + HD32_EVAL_ONLY)
        # teacher-score term: total = loss(logits, labels) + distill_alpha * kd(logits[:, :nway], batch["teacher_scores"]); distill_only drops
        # the first summand.  last_kd: the unweighted term of the last step (device scalar, like last_reg)
        self.distill, self.distill_alpha, self.distill_T, self.distill_only = distill, float(distill_alpha), float(distill_T), bool(distill_only)
        self.last_kd = None
        self.model = model
        # the scorer is the model's (NwayDualEncoder(cosine=..., cosine_scale=...)): cosine_scale * cosine similarity instead of the dot product;
        # everything behind the logits is the same
        self.cosine, self.cosine_scale = bool(getattr(model, "cosine", False)), float(getattr(model, "cosine_scale", 1.0))
        self.loss_kind, self.T = loss, T
        self.reg_lambda = float(reg_lambda)
        self.last_reg = None
        self.lr0, self.wd, self.eps, self.max_grad_norm = learning_rate, weight_decay, adam_epsilon, max_grad_norm
        self.warmup_steps, self.total_steps, self.betas = warmup_steps, total_steps, betas
        self.global_step = 0
        self.adam_step = 0          # bias-correction step of AdamW: differs from global_step only after resuming a reference fp16
                                    # checkpoint whose GradScaler skipped steps (state["step"] < global_step there)
        # CLDRD_FORCE_DDP=1: take the data-parallel path (constructor broadcast, bucket hooks, communication stream, Work handles) with a
        # process group of ONE rank too - the only way to run it over RCCL (ProcessGroupNCCL) on a one-GPU box (tests/test_gpu_ddp.py)
        self.distributed = dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _env_flag("CLDRD_FORCE_DDP", "0") == "1")
        self.world = dist.get_world_size() if self.distributed else 1
        self.flat_p, self.flat_g = model.fuse_flat()
        # --deterministic: the embedding-table gradients - the one part of the step summed by float atomics - become fixed-order per-row sums
        # (encoder.HipEncoder.deterministic_embed): the same batches then give the same bits, run after run, eager or replayed
        self.deterministic = bool(deterministic)
        for t in model.towers():
            t.deterministic_embed = self.deterministic
        # deferred weight gradients: one group launch per tower at the end of the backward on one GPU; with RCCL every
        # ceil(layers / 2) layers, so the first half of the buckets is all-reduced while the rest of the backward still runs
        for t in model.towers():
            t.wgrad_flush_layers = max(1, -(-t.cfg.n_layers // 2)) if self.distributed else 0
        dev = self.flat_p.device
        self._require_gpu(dev)
        n = self.flat_p.numel()
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        # weight-decay flag per 64-parameter chunk (every parameter starts on a 64 boundary)
        flags = torch.zeros(n // 64, dtype=torch.uint8)
        self.buckets = []          # (tower index, layer index or -1, start, end) in joint-flat coordinates
        for ti, (tower, toff) in enumerate(zip(model.towers(), model._tower_offsets)):
            for name in tower.layout.order:
                off, shape = tower.layout.entries[name]
                numel = math.prod(shape)
                prefix = "query_encoder." if ti == 0 else "passage_encoder."
                if not no_decay(prefix + name):
                    flags[(toff + off) // 64:(toff + off + numel + 63) // 64] |= 1
                if name.startswith("embeddings.") and name.endswith("_embeddings.weight"):
                    # bit 1: no bf16 / fp16 shadow (cldrd_adamw_step): the embedding kernels read the fp32 tables
                    flags[(toff + off) // 64:(toff + off + numel + 63) // 64] |= 2
            for li, (a, b) in enumerate(tower.layout.layer_range):
                self.buckets.append((ti, li, toff + a, toff + b))
            a, b = tower.layout.embed_range
            self.buckets.append((ti, -1, toff + a, toff + b))
        self.decay_flags = flags.to(dev)
        self.clip = torch.zeros(3, dtype=torch.float32, device=dev)
        self._norm = _ClipNormPlan(model, self.flat_g)
        self.norm_partial = self._norm.partial
        self.comm_stream = torch.cuda.Stream(device=dev) if self.distributed else None
        if self.comm_stream is not None:
            self.flat_g.record_stream(self.comm_stream)        # the bucket slices are used on it (the buffer lives as long as the trainer)
        # the query tower's stream, at the priority of torch's current stream (a high-priority stream changed nothing: profiles/r03_microbench.txt)
        self.q_stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        # third stream: scoring + loss + score backward between the towers' forward and backward (see forward_backward)
        self.l_stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        self._pending = []
        # HIP-graph replay of the step (see train_step).  `_state`: None, or the device words a captured step reads - {"seeds": int64[2], the
        # towers' dropout seeds, "hyper": float32[2], {lr, Adam step size}} - from the first capture on; `_graphs`: batch key -> what `_capture`
        # returned for that shape; `_policy`: which step is captured / replayed (a failed capture: every later step runs eagerly)
        self._state = None
        self._graphs = {}
        self._policy = _CapturePolicy(self._DDP_WARM, self.distributed)
        self.last_logits = None
        # test hooks (tests/test_gpu_model.py, test_gpu_amp16.py prove the default path equal to the plain one they select; not configuration):
        self.zero_all_grads = False        # True: zero the whole gradient buffer and accumulate instead of writing every gradient once
        self.use_norm_sink = True          # False: the late clip-norm piece by a separate pass over the gradients
        # CLDRD_AMP=fp16 towers (encoder.py: amp16): the loss scale lives in device memory (hip_ops.new_loss_scale_state).  It is set every
        # step from dL/dCLS (ops.loss_scale_adapt: a power of two that puts the largest entering gradient at 2^11..2^12); what is kept of
        # torch.cuda.amp.GradScaler (the reference: nway_listwise_1.py:355-359) is its safety net: a non-finite gradient norm skips the step
        # and backs the scale off, `scale_growth_interval` (GradScaler's default 2000) finite steps give a factor 2 back.
        self.amp16 = any(getattr(t, "amp16", False) for t in model.towers())
        self.scale_growth_interval = 2000
        self._scale_state = ops.new_loss_scale_state(dev) if self.amp16 else None
        # device {lr, Adam step size} of the eager loss-scaled step (see _optimizer_launches)
        self._hyper = torch.zeros(2, dtype=torch.float32, device=dev) if self.amp16 else None
        self._opt_step_loaded = None       # Adam's step count of the optimizer state loaded last (load_state_dict)
        if self.distributed:
            # DDP constructor semantics (reference :250-255): rank 0's parameters win
            dist.broadcast(self.flat_p, src=0)
            dist.barrier()
        self._build_shadows()

    @staticmethod
    def _require_gpu(dev):
        if dev.type != "cuda":
            raise RuntimeError("NwayTrainer needs the model on a GPU (no CPU path)")

    # ---------------------------------------------------------------------------------------------------------
    def lr(self, step=None) -> float:
        step = self.global_step if step is None else step
        return self.lr0 * linear_schedule_factor(step, self.warmup_steps, self.total_steps)

    def _bucket_hook(self, ti):
        if not self.distributed:
            return None
        index = {(b[0], b[1]): (b[2], b[3]) for b in self.buckets}

        def hook(layer):
            # The bucket's gradients are complete on the stream the hook is called on: the communication stream waits for exactly
            # that point, then the all-reduce is issued ASYNCHRONOUSLY from it and its Work handle kept.  Nothing here relies on what a
            # blocking collective does to the caller's stream (ProcessGroupNCCL makes the current stream wait for its internal one,
            # gloo blocks the host): `_wait_pending` below is the one place where the result is ordered before its consumer.
            a, b = index[(ti, layer)]
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                work = dist.all_reduce(self.flat_g[a:b], op=dist.ReduceOp.SUM, async_op=True)
            self._pending.append(work)
        return hook

    def _wait_pending(self):
        """Order every outstanding bucket all-reduce before whatever the CURRENT stream runs next (the gradient norm / optimizer):
        ``Work.wait()`` makes the current stream wait for the collective under ProcessGroupNCCL (no host block) and blocks the host
        until completion under gloo; the stream-level join with the communication stream covers the copies gloo does on it."""
        pending, self._pending = self._pending, []
        for w in pending:
            w.wait()
        if self.comm_stream is not None:
            torch.cuda.current_stream().wait_stream(self.comm_stream)

    def forward_backward(self, batch, _state_written=False):
        """Runs forward + backward (+ overlapped gradient all-reduce).  Returns (loss_out[2] device tensor, logits)."""
        model = self.model
        if self._state is not None and not _state_written and not torch.cuda.is_current_stream_capturing():
            # called on its own (tests, custom loops) while the towers read their dropout seeds from device memory: fresh seeds first
            self._write_step_state()
        qe, pe = model.query_encoder, model.passage_encoder
        q, nw = batch["query"], batch["nway_passages"]
        bz, nway, L = nw["input_ids"].shape
        teacher = self._teacher_scores(batch, bz, nway)
        pids = self._nway_pids(batch, bz, nway)
        write_once = not model.share_weights and not self.zero_all_grads      # (test hook: zero_all_grads = True zeroes + accumulates)
        main = torch.cuda.current_stream()
        # The query tower is ~1 % of the FLOPs but dozens of small, latency-bound launches: it runs on its own stream
        # next to the passage tower (forward and backward) instead of in front of it.
        side = self.q_stream if (not model.share_weights and self.q_stream is not None) else main
        if side is not main:
            side.wait_stream(main)
        # Step preamble that nothing in the passage tower's FORWARD depends on - on the second stream, next to that forward instead of in
        # front of it (134 us of a 12-ms step on the main stream until round 3, profiles/r03_microbench.txt): the zeros the embedding
        # tables' scatter-adds need and the transposed weight copies of the data-gradient GEMMs (left stale by the optimizer step).  The
        # main stream joins the second one after the forward, long before the backward reads either.
        with torch.cuda.stream(side):
            if not write_once:
                self.flat_g.zero_()                 # two tapes accumulate into one tower's gradients
            else:
                # every weight / bias / LayerNorm gradient is written exactly once per step (accumulate=False below); only the
                # embedding tables are scatter-added into and need zeros (2 x 94 MB instead of the whole 531 MB buffer)
                ops.zero_segments([self.flat_g[toff + t.layout.embed_range[0]:toff + t.layout.embed_range[1]]
                                   for t, toff in zip(model.towers(), model._tower_offsets)])      # one launch for both towers' tables
            for tower in model.towers():
                if not tower._t_fresh:
                    tower.refresh_transposed()
        # (The query tower enqueued in slices, each released at one of the passage tower's HBM-bound kernels, was measured 5-8 % slower than
        # this free-running schedule and removed: profiles/r06_microbench.txt section 1.)
        p_ids, p_mask = nw["input_ids"].reshape(bz * nway, L), nw["attention_mask"].reshape(bz * nway, L)
        with torch.cuda.stream(side):
            q_cls, q_tape = qe.encode(q["input_ids"], q.get("attention_mask"), train=True, save=True, fp16=model.query_fp16, device_seed=True)
        p_cls, p_tape = pe.encode(p_ids, p_mask, train=True, save=True, fp16=False, lengths=_lengths(nw), device_seed=True)      # "lengths" given: a packed batch
        if side is not main:
            main.wait_stream(side)
            q_cls.record_stream(main)
        mode = score_mode(model.in_batch_loss, model.all_in_batch_neg)
        Np = ops.score_cols(bz, nway, mode)
        # Scoring, loss and score backward on a stream of their OWN between the two joins.  In a replayed HIP graph a cross-stream edge is
        # honoured when the source stream's run of consecutive nodes ENDS, not at the node the edge leaves from: with the loss kernels on the
        # main stream the executor kept them and the query tower's backward (the branch captured first) in one run on one hardware queue, and
        # the passage tower's backward - the critical path - started only when that run was over: 0.62 ms of 5-10-us kernels with the rest of
        # the chip idle (kernel trace of the replayed step, profiles/r04_microbench.txt section 14).  A run that contains nothing but the loss
        # ends where both towers' backward begin.
        lst = self.l_stream if (side is not main and self.l_stream is not None) else main
        if lst is not main:
            lst.wait_stream(main)
        with torch.cuda.stream(lst):
            logits = torch.empty(bz, Np, dtype=torch.float32, device=q_cls.device)
            if self.cosine:
                inv_norms = torch.empty(bz + bz * nway, dtype=torch.float32, device=q_cls.device)
                ops.score_cos_fwd(q_cls, p_cls, logits, inv_norms, bz, nway, mode, self.cosine_scale)
            else:
                ops.score_fwd(q_cls, p_cls, logits, bz, nway, mode)
            labels = batch["labels"].to(device=logits.device, dtype=torch.float32)
            if mode != 0:   # in-batch negatives get the -0.5 label (reference nway_listwise_1.py:341-344)
                labels = torch.cat([labels, torch.full((bz, Np - nway), -0.5, dtype=torch.float32, device=logits.device)], dim=-1)
            if self.distill_only:
                loss_out, dlogits = torch.zeros(2, dtype=torch.float32, device=logits.device), torch.zeros_like(logits)
            elif self.loss_kind == "lambda_loss":
                loss_out, dlogits = torch.empty(2, dtype=torch.float32, device=logits.device), torch.empty_like(logits)
                if self.label_source == "teacher":
                    labels = teacher.to(device=logits.device, dtype=torch.float32)
                ops.lambda_term(logits, labels.contiguous(), loss_out, dlogits, **self._lambda_kw)
            elif self.loss_kind in CONTRASTIVE_KINDS:
                loss_out, dlogits = torch.empty(2, dtype=torch.float32, device=logits.device), torch.empty_like(logits)
                ops.softmax_ce(logits, labels.contiguous(), loss_out, dlogits, mode=mode, nway=nway,
                               pids=None if pids is None else pids.to(device=logits.device, dtype=torch.int64).contiguous(), **self._ce_kw)
            else:
                loss_out, dlogits = ops.loss_fwd_bwd(self.loss_kind, logits, labels.contiguous(), T=self.T)
            if self.reg_lambda > 0.0 and mode == 0:     # reference nway_listwise_1.py:346-350: only without in-batch negatives
                self.last_reg = torch.empty(1, dtype=torch.float32, device=logits.device)
                ops.logit_norm_reg(logits, self.reg_lambda, loss_out, dlogits, self.last_reg)
            if self.distill is not None:
                # the row's own nway columns only: the in-batch columns behind them have no teacher score and keep the rank loss's gradient
                self.last_kd = torch.empty(1, dtype=torch.float32, device=logits.device)
                ops.distill_term(self.distill, logits, teacher.to(device=logits.device, dtype=torch.float32).contiguous(), self.distill_alpha,
                                 self.distill_T, loss_out, dlogits, self.last_kd)
            if self.world > 1:
                dlogits.mul_(1.0 / self.world)      # gradient mean over ranks == DDP's all-reduce / world_size
            dq, dp = torch.empty_like(q_cls), torch.empty_like(p_cls)
            if self.cosine:
                ops.score_cos_bwd(dlogits, logits, q_cls, p_cls, inv_norms, dq, dp, bz, nway, mode, self.cosine_scale)
            else:
                ops.score_bwd(dlogits, q_cls, p_cls, dq, dp, bz, nway, mode)
            if self.amp16:
                ops.loss_scale_adapt(dq, dp, self._scale_state)          # dq, dp leave multiplied by S; every fp16 gradient downstream carries it
        if lst is not main:
            main.wait_stream(lst)
            for t_ in (logits, loss_out, dq, dp, q_cls, p_cls):
                t_.record_stream(main)
            q_cls.record_stream(lst)
            p_cls.record_stream(lst)
        with self._loss_scale():
            self._backward(q_tape, p_tape, dq, dp, main, side, lst, write_once)
        return loss_out, logits

    def _reads_teacher_scores(self) -> bool:
        return self.distill is not None or self.label_source == "teacher"

    def _teacher_scores(self, batch, bz, nway):
        """batch["teacher_scores"] of a trainer that distils or takes its labels from the teacher ([B, nway], checked); None for any other
        trainer (the key is ignored)."""
        if not self._reads_teacher_scores():
            return None
        t = batch.get("teacher_scores")
        if not isinstance(t, torch.Tensor):
            why = f"distils ({self.distill})" if self.distill is not None else "takes its labels from the teacher (label_source)"
            raise ValueError(f"this trainer {why} and needs batch['teacher_scores'] (float [B, nway]): build the training "
                             "file with dataset.curriculum_file --with_scores and the dataset with teacher_scores=True")
        if tuple(t.shape) != (bz, nway):
            raise ValueError(f"batch['teacher_scores'] must be [{bz}, {nway}] like the passages, got {tuple(t.shape)}")
        return t

    def _reads_nway_pids(self) -> bool:
        return self.ce_mask_duplicate_pids and not self.distill_only

    def _nway_pids(self, batch, bz, nway):
        """batch["nway_pids"] of a trainer that masks duplicate passages (int64 [B, nway], checked); None for any other trainer."""
        if not self._reads_nway_pids():
            return None
        p = batch.get("nway_pids")
        if p is not None and not isinstance(p, torch.Tensor):
            p = torch.as_tensor(p)               # collate_fn returns the ids as a numpy array
        if p is None:
            raise ValueError("this trainer masks duplicate passages (ce_mask_duplicate_pids) and needs batch['nway_pids'] (int64 [B, nway], the "
                             "passage ids NwayDataset.collate_fn returns); synthetic batches have none")
        if tuple(p.shape) != (bz, nway) or p.dtype != torch.int64:
            raise ValueError(f"batch['nway_pids'] must be int64 [{bz}, {nway}] like the passages, got {p.dtype} {tuple(p.shape)}")
        return p

    def _backward(self, q_tape, p_tape, dq, dp, main, side, lst, write_once):
        """both towers' backward from dq / dp (scaled by the loss scale in the amp16 mode) + the bucket all-reduces.  ``main``, ``side``, ``lst``:
        the streams of the passage tower, the query tower and the loss (forward_backward; any of the last two may be ``main`` itself)."""
        qe, pe = self.model.query_encoder, self.model.passage_encoder
        self._norm.begin_step()
        if self.model.share_weights:
            # one tower, two tapes: gradients accumulate; all-reduce once everything is in
            pe.backward_from_cls(p_tape, dp)
            qe.backward_from_cls(q_tape, dq)
            if self.distributed:
                dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM)
        else:
            def query_backward():
                if side is not main:
                    side.wait_stream(lst)
                    dq.record_stream(side)
                with torch.cuda.stream(side):
                    qe.backward_from_cls(q_tape, dq, after_layer=self._bucket_hook(0), accumulate=not write_once)
            # The query tower's ~150 small backward launches run next to the passage tower's data-gradient chain.  (Next to its LAST
            # weight-gradient group instead - one ~3-ms launch off the critical path - measured +1.2 % step time, profiles/r03_microbench.txt:
            # that group loses more to the intruders than the GEMM chain does; the switch for it was removed in round 4.)
            # Order of the two towers' backward.  Eager: the query tower first - its ~150 small launches then run next to the passage tower's
            # data-gradient chain (enqueued behind ~150 passage launches they would start late and land on the last weight-gradient group:
            # +1.2 %, round 3).  Under GRAPH CAPTURE the order decides something else: the branch captured first behind the fork continues on
            # the hardware queue that ran the loss, the other one is released late - with the query tower first, the passage tower's backward
            # (the critical path) sat idle for 0.62 ms behind the loss in every replayed step (kernel trace, profiles/r04_microbench.txt
            # section 14).  So a captured step enqueues the passage tower first; the query tower's chain is released ~1.8 ms behind the loss
            # and still ends 4 ms before the join.
            q_late = side is not main and torch.cuda.is_current_stream_capturing()
            if not q_late:
                query_backward()
            p_hook = self._bucket_hook(1)
            if p_hook is None and side is not main and write_once:
                # one GPU: the clip norm in two pieces (_ClipNormPlan; test hook: use_norm_sink = False takes the late piece by a separate pass)
                p_hook = self._norm.early_hook(main, side, defer=q_late, use_sink=self.use_norm_sink)
            pe.backward_from_cls(p_tape, dp, after_layer=p_hook, accumulate=not write_once)
            if q_late:
                # (released together with the passage tower's last weight-gradient group instead: +1.4 %, as in round 3's eager measurement)
                query_backward()
                self._norm.enqueue_early()
            main.wait_stream(side)
            if self.distributed:
                self._wait_pending()

    # ---- the step's host bookkeeping: ONE place advances the counters, ONE draws and writes the device-side step state -------------
    def _advance_counters(self):
        """global_step / adam_step of the step that is about to be applied; -> the lr in effect during it (the scheduler steps afterwards)."""
        self.global_step += 1
        self.adam_step += 1
        return self.lr(self.global_step - 1)

    def _write_step_state(self, lr=None):
        """Draw the towers' dropout seeds of this step and write them to device memory (`_state`), in stream order in front of the launches
        that read them; with ``lr`` also {lr, Adam step size} of step ``adam_step`` (less the steps the loss-scale safety net skipped)."""
        seeds = [t.next_seed() for t in self.model.towers()]
        hyper = lr is not None
        ops.write_step_state(self._state["seeds"], seeds[0], seeds[1] if len(seeds) > 1 else 0, self._state["hyper"] if hyper else None,
                             lr if hyper else 0.0, self.betas[0], self.betas[1], self.adam_step if hyper else 1,
                             scale_state=self._scale_state if hyper else None)

    def _advance_step_state(self):
        """A step whose launches read their seeds, lr and Adam step size from device memory (a replay, or an eager step while a captured
        shape exists): the counters, then the one small launch that writes this step's values.  Returns lr."""
        lr = self._advance_counters()
        self._write_step_state(lr)
        return lr

    def optimizer_step(self):
        """clip_grad_norm_ + AdamW + scheduler.step of reference nway_listwise_1.py:355-367.  What is kept of its GradScaler (fp16 mode; the
        bf16 mode has no loss scale) is the safety net: a non-finite gradient norm skips the step on the device."""
        lr = self._advance_counters()
        self._optimizer_launches(lr, self.adam_step)
        return lr

    def _loss_scale(self):
        """Launch context of the loss-scaled (fp16) mode: the backward unscales by, and the clip coefficient updates, the device scale."""
        return ops.loss_scale(self._scale_state.data_ptr() if self.amp16 else None, self.scale_growth_interval)

    def _optimizer_launches(self, lr, adam_step):
        """The device work of one optimizer step.  Under a captured step (`_state` installed) lr and the bias-corrected step size are
        read from device memory at replay time and the by-value arguments given here are ignored by the kernel."""
        with self._loss_scale():     # clip_coef updates the scale
            self._norm_launches()
        towers = self.model.towers()
        hyper = self._state["hyper"] if self._state else None
        if hyper is None and self.amp16:
            # eager step of the loss-scaled mode: {lr, step size} go through device memory too, because the bias-correction exponent
            # is adam_step MINUS the steps the safety net skipped, and that count lives on the device (`_scale_state[3]`, updated by the
            # clip_coef launch just above; a skipped step leaves p / m / v untouched, so its own step size does not matter)
            hyper = self._hyper
            ops.write_step_state(None, 0, 0, hyper, lr, self.betas[0], self.betas[1], adam_step, scale_state=self._scale_state)
        self._adamw_launches(lr, adam_step, towers, hyper)

    @property
    def _sink_on(self):
        return self._norm.sink_on

    def _norm_launches(self):
        self._norm.launch(self.flat_g, self.max_grad_norm, self.clip)

    def _adamw_launches(self, lr, adam_step, towers, hyper=None):
        # one AdamW launch over the joint buffer; it also writes the 16-bit weight shadows: the fp16 one of the towers whose forward reads fp16
        # weights (one contiguous range of the joint buffer) and the bf16 one - unless no pass of a training step reads it (`_skip_h`)
        s16, r16, skip_h = self._shadow16, self._shadow16_range, self._skip_h
        fused16 = s16 is not None
        with ops.optim_hyper(hyper.data_ptr() if hyper is not None else None):
            ops.adamw_step(self.flat_p, self.flat_g, self.m, self.v, self.decay_flags, None if skip_h else self._shadow, lr=lr, beta1=self.betas[0],
                           beta2=self.betas[1], eps=self.eps, weight_decay=self.wd, step=adam_step, clip=self.clip,
                           shadow16=s16[r16[0]:r16[1]] if fused16 else None, h16_range=r16 if fused16 else None)
        # the transposed copies wait for the next step's preamble on the second stream (forward_backward) when there is one
        defer_t = not self.model.share_weights and self.q_stream is not None
        for t in towers:
            t.refresh_shadows(need_transposed=not defer_t, cast=False, cast16=not fused16, h_stale=skip_h)

    def _build_shadows(self):
        """The joint 16-bit weight shadows AdamW writes, once per trainer: bf16 over the whole joint buffer (each tower's ``flat_h`` a slice) and
        fp16 over the towers that read fp16 weights - adjacent in the joint buffer, so one range covers them (``flat_h16`` a slice each)."""
        towers, offs = self.model.towers(), self.model._tower_offsets
        n, dev = self.flat_p.numel(), self.flat_p.device
        self._shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
        self._shadow16, self._shadow16_range = None, None
        need = [(t, off) for t, off in zip(towers, offs) if t.needs_h16]
        if need:
            lo, hi = need[0][1], need[-1][1] + need[-1][0].layout.total
            if sum(t.layout.total for t, _ in need) != hi - lo:
                raise RuntimeError("towers with fp16 weights are not adjacent in the joint buffer")
            self._shadow16, self._shadow16_range = torch.empty(n, dtype=torch.float16, device=dev), (lo, hi)
            for t, off in need:
                t.flat_h16 = self._shadow16[off:off + t.layout.total]
                t._shadow_version = -1
        # all-fp16 training: no pass of a training step reads the bf16 shadow (forward, backward and the transposed copies come from the fp16
        # one), so AdamW does not write it; the towers remember it is stale and an evaluation forward casts it first
        self._skip_h = bool(self.amp16 and all(t.amp16 for t in towers) and self._shadow16 is not None)
        for t, off in zip(towers, offs):
            t.flat_h = self._shadow[off:off + t.layout.total]
            t.refresh_shadows(need_transposed=True)

    def train_step(self, batch):
        """One full step; returns the device tensor {loss, pair count} (no host sync).

        After `_DDP_WARM` (3) eager steps on one batch shape the step - forward, loss, backward, clip, AdamW, shadows, all three
        streams: ~370 kernel launches - is captured into a HIP graph and replayed (``CLDRD_GRAPH=0``: always eager; `_CapturePolicy`: which
        steps, on one GPU and under torch.distributed).  The host then spends ~0.1 ms per step instead of ~3.7 ms,
        which is what an enqueue-bound shape (cfg1: B = 4, N = 8) and eight rank processes sharing one host need.  What changes
        from step to step - the two towers' dropout seeds, lr, Adam's bias-corrected step size - lives in device memory and is
        written by one small launch in front of each replay (``ops.write_step_state``); results are bit-identical to the eager path."""
        nw = batch["nway_passages"]
        lens = _lengths(nw)
        if lens is not None:
            bz_, nway_, L_ = nw["input_ids"].shape
            if not self.model.passage_encoder.would_pack(lens, bz_ * nway_, L_, has_mask=nw.get("attention_mask") is not None):
                # "lengths" came with the batch (batch_to_device attaches them to every right-padded batch) but the encoder will not pack it
                # (fill above 92 %, CLDRD_PACK=0): it is an ordinary padded batch and takes the graph path like one
                batch = dict(batch.items())
                batch["nway_passages"] = {k: v for k, v in nw.items() if k != "lengths"}
                lens = None
        if self._graph_wanted():
            out = self._train_step_graph(batch, padded=lens is None)       # a packed batch changes its row count every step: eager
            if out is not None:
                return out
        if self._state is not None:
            # a captured shape exists, so the towers read their seeds (and AdamW its lr) from device memory: an eager step (another
            # batch shape) writes this step's values there first, exactly as a replay does
            lr = self._advance_step_state()
            loss_out, logits = self.forward_backward(batch, _state_written=True)
            self._optimizer_launches(lr, self.adam_step)
        else:
            # the plain eager step: the towers draw their own seeds, the hyper-parameters go by value, the counters advance after the backward
            loss_out, logits = self.forward_backward(batch)
            self.optimizer_step()
        self.last_logits = logits
        return loss_out

    def skipped_steps(self) -> int:
        """Steps the loss-scale safety net skipped so far (a device -> host read: logging / checkpoint time only)."""
        return int(self._scale_state[3].item()) if self._scale_state is not None else 0

    # ---- HIP-graph replay of the step --------------------------------------------------------------------------------------
    _DDP_WARM = 3               # eager steps in front of the capture (and, under torch.distributed, in front of the agreement step)

    @property
    def _ddp_steps(self):
        """train_step calls under torch.distributed while a graph was wanted (the agreement happens at a fixed count)"""
        return self._policy.calls

    @property
    def _graph_broken(self):
        return self._policy.broken

    def _graph_wanted(self):
        if self.distributed:
            # data-parallel ranks: the bucket all-reduces are issued from hooks INSIDE the step.  Over ProcessGroupNCCL (= RCCL) they can be
            # captured with it (the collective's launch is recorded on its stream, Work.wait() becomes an event edge of the graph); gloo
            # (tests) copies through the host and cannot.  With MORE THAN ONE rank this is opt-in (CLDRD_DDP_GRAPH=1): capture + replay of
            # collectives has only ever run with one rank on this pool (one GPU per box), so real multi-rank jobs launch eagerly by default;
            # a one-rank process group (CLDRD_FORCE_DDP: the bench's ddp leg, tests) captures by default.
            if _env_flag("CLDRD_DDP_GRAPH", "1" if self.world == 1 else "0") != "1" or dist.get_backend() != "nccl":
                return False
        return (not self.model.share_weights and not self._graph_broken
                and _env_flag("CLDRD_GRAPH", "1") != "0" and self.flat_p.is_cuda)

    def _step_inputs(self, batch):
        """The per-step inputs of the captured step: [(where it sits in the batch dict, tensor, dtype the static batch holds it in - None: its
        own)], in ONE order for the batch key, the static batch and every incoming one (at most 7 segments; cldrd_copy_segments takes 8).
        The teacher scores are one of them, once: a step that distils or takes its labels from the teacher reads this step's scores; so are
        the passage ids of a step that masks duplicate passages."""
        q, nw = batch["query"], batch["nway_passages"]
        items = [(("query", "input_ids"), q["input_ids"], None), (("nway_passages", "input_ids"), nw["input_ids"], None),
                 (("nway_passages", "attention_mask"), nw["attention_mask"], None), (("labels",), batch["labels"], torch.float32)]
        if q.get("attention_mask") is not None:
            items.append((("query", "attention_mask"), q["attention_mask"], None))
        if self._reads_teacher_scores():
            bz, nway, _ = nw["input_ids"].shape
            items.append((("teacher_scores",), self._teacher_scores(batch, bz, nway), torch.float32))
        if self._reads_nway_pids():
            bz, nway, _ = nw["input_ids"].shape
            items.append((("nway_pids",), self._nway_pids(batch, bz, nway), None))
        return items

    def _batch_key(self, batch):
        return tuple((where, tuple(t.shape)) for where, t, _ in self._step_inputs(batch))

    def _train_step_graph(self, batch, padded=True):
        """Ask the policy what this step is and carry the answer out; -> the step's loss tensor, or None: the caller runs it eagerly."""
        P = _CapturePolicy
        key = self._batch_key(batch) if padded else None
        action = self._policy.decide(key, padded)
        if action == P.VOTE_NO:
            self._policy.record(key, self._agree_on_capture(False))       # (not eligible at the agreement step: every rank stays eager for good)
        if action in (P.EAGER, P.VOTE_NO):
            return None
        towers = self.model.towers()
        if action == P.CAPTURE:
            if self._state is None:
                dev = self.flat_p.device
                self._state = {"seeds": torch.zeros(2, dtype=torch.int64, device=dev), "hyper": torch.zeros(2, dtype=torch.float32, device=dev)}
            entry = None
            try:
                entry = self._capture(batch)
            except Exception as exc:       # a capture problem must never take training down: fall back to the eager step for good
                import warnings
                first = exc
                while first.__context__ is not None:          # what went wrong INSIDE the capture (the capture's own exit error hides it)
                    first = first.__context__
                warnings.warn(f"HIP-graph capture of the training step failed ({type(first).__name__}: {first}); staying eager")
            ok = entry is not None
            if self.distributed:    # (a one-rank forced group, CLDRD_FORCE_DDP, takes the same path: the agreement is then a one-rank all-reduce)
                ok = self._agree_on_capture(ok)
            self._policy.record(key, ok)
            if not ok:
                for t in towers:
                    t.seed_base_ptr = None
                    t._t_fresh = False       # refresh_transposed() inside the failed capture set the flag without executing a kernel
                self._state = None
                self._norm.begin_step()
                torch.cuda.synchronize()
                return None
            self._graphs[key] = entry
        entry = self._graphs[key]
        # this step's inputs and state, in stream order in front of the replay
        dsts, srcs = entry["inputs"], [t for _, t, _ in self._step_inputs(batch)]
        if all(s_.is_cuda and s_.is_contiguous() and s_.dtype == d_.dtype and s_.shape == d_.shape for d_, s_ in zip(dsts, srcs)):
            ops.copy_segments(dsts, srcs)           # one launch instead of five
        else:
            for dst, src in zip(dsts, srcs):
                dst.copy_(src, non_blocking=True)
        self._advance_step_state()
        entry["graph"].replay()
        if self._skip_h:
            # The captured AdamW skipped the bf16 weight shadow (all-fp16 training reads none of it).  The Python call that records this
            # (refresh_shadows(h_stale=True)) ran at capture time only; a replay changes the weights again, so every replay has to leave the
            # towers marked - or an evaluation forward after further replays would encode with the bf16 matrices of the LAST evaluation.
            for t in towers:
                t._h_stale = True
        self.last_logits = entry["logits"]
        if self.distill is not None:
            self.last_kd = entry["last_kd"]          # this shape's captured output (another shape's replay or an eager step may have run since)
        return entry["loss_out"]

    def _agree_on_capture(self, ok: bool) -> bool:
        """MIN over ranks of "my capture worked" (one small all-reduce + a host read, once per job)."""
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.flat_p.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        agreed = bool(int(flag.item()))
        if not agreed and ok:
            import warnings
            warnings.warn("HIP-graph capture of the training step failed on another rank; every rank stays eager")
        return agreed

    def _capture(self, batch):
        dev = self.flat_p.device
        static = {}
        for where, t, dtype in self._step_inputs(batch):
            d = static
            for k in where[:-1]:
                d = d.setdefault(k, {})
            d[where[-1]] = t.to(device=dev, dtype=dtype or t.dtype).contiguous().clone()
        for i, t in enumerate(self.model.towers()):
            t.seed_base_ptr = self._state["seeds"].data_ptr() + 8 * i
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        # the captured launches take seeds / lr from device memory: nothing of THIS step's values is baked in (the counters are not
        # advanced here; the capture itself executes nothing)
        # thread_local: only THIS thread's calls are checked against the capture.  The default ("global") makes any HIP call of any other thread
        # an error while the capture runs - and a process with a ProcessGroupNCCL has such a thread: the watchdog polls the events of earlier
        # collectives (seen as a 1-in-3 failure of the one-rank RCCL test when the whole suite ran before it).
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            try:
                loss_out, logits = self.forward_backward(static)
                self._optimizer_launches(0.0, 1)
            except BaseException:
                # join every stream forked inside the capture before it ends: otherwise ending it fails too ("unjoined work"), the stream
                # stays in capture mode and the eager fallback cannot run either
                cur = torch.cuda.current_stream()
                for s_ in (self.q_stream, self.l_stream, self.comm_stream):
                    if s_ is not None:
                        cur.wait_stream(s_)
                raise
        return {"graph": g, "inputs": [t for _, t, _ in self._step_inputs(static)], "loss_out": loss_out, "logits": logits, "static": static,
                "last_kd": self.last_kd}

    # ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def train_metrics(self, logits, labels, topk: int = 10):
        """Per-batch train MRR@k / Recall@k w.r.t. the ``labels == 1`` position (reference :375-385); call on logging steps."""
        order = torch.argsort(logits.float(), dim=-1, descending=True, stable=True)
        lab = torch.gather(labels.to(logits.device).float(), 1, order).cpu().numpy()
        import numpy as np
        first = np.where(lab == 1)[1]
        keep = first[first < topk]
        if len(keep) == 0:
            return 0.0, 0.0
        return float(np.sum(1.0 / (keep + 1.0)) / len(first)), float(len(keep) / len(first))

    def metric_labels(self, batch, n_cols: int):
        """The labels `train_metrics` ranks against, [B, n_cols] (in-batch columns: -0.5).  label_source "teacher": no label equals 1 there,
        so the column with the highest teacher score of a row is its relevant one."""
        if self.label_source == "teacher":
            t = batch["teacher_scores"]
            labels = torch.zeros(t.shape, dtype=torch.float32, device=t.device).scatter_(1, t.argmax(dim=1, keepdim=True), 1.0)
        else:
            labels = batch["labels"]
        if n_cols != labels.shape[1]:
            labels = torch.cat([labels, torch.full((labels.shape[0], n_cols - labels.shape[1]), -0.5, device=labels.device)], dim=-1)
        return labels

    # ---- validation on a dev run (the reference's launch scripts pass --dev_path ...; its trainers import RerankingEvaluator) --
    def validate(self, pool, evaluator, batch_size: int = 512) -> dict:
        """The metrics of ``evaluator`` (evaluation.RerankingEvaluator) for the student as it stands, re-ranking the dev run ``pool``
        (evaluation.DevPool).  Training goes on as if it had not been called: an evaluation pass writes no parameter, moment or gradient
        and no step state; the evaluator puts ``model.training`` and the towers' dropout step counters back; the evaluation forward
        launches eagerly from the ordinary allocator, so the captured graphs (their private memory pool, their static inputs) stay as they
        are and the next step of a captured shape is a replay.  The weight shadows need nothing new: an evaluation forward casts what is
        stale before it reads it (HipEncoder._shadows_ok), and the next step - `_adamw_launches`, or the replay site of
        `_train_step_graph` - marks the bf16 shadow stale again."""
        return evaluator.compute_metrics_pool(self.model, pool, batch_size=batch_size)

    # ---- checkpoint payload (reference nway_listwise_1.py:418-426 / :300-304) --------------------------------------------
    def _optimizer_names(self):
        return optimizer_param_groups(self.model)

    def _slice(self, buf, ti, hf_name):
        tower, toff = self.model.towers()[ti], self.model._tower_offsets[ti]
        off, shape = tower.layout.entries[hf_name]
        return buf[toff + off:toff + off + math.prod(shape)].view(shape)

    def optimizer_state_dict(self):
        """``torch.optim.Optimizer.state_dict()`` layout of the reference's AdamW (state: step / exp_avg / exp_avg_sq per parameter
        index; two param groups), so a reference run can resume from a checkpoint written here and vice versa."""
        groups = self._optimizer_names()
        state, param_groups, idx = {}, [], 0
        applied = max(0, self.adam_step - self.skipped_steps())      # scaler.step() semantics: skipped steps do not count (reference :357)
        for gi, entries in enumerate(groups):
            ids = []
            for _, ti, n in entries:
                if ti is not None and applied > 0:
                    state[idx] = {"step": applied, "exp_avg": self._slice(self.m, ti, n).detach().cpu().clone(),
                                  "exp_avg_sq": self._slice(self.v, ti, n).detach().cpu().clone()}
                ids.append(idx)
                idx += 1
            param_groups.append({"weight_decay": self.wd if gi == 0 else 0.0, "lr": self.lr(), "initial_lr": self.lr0,
                                 "betas": tuple(self.betas), "eps": self.eps, "correct_bias": True, "params": ids})
        return {"state": state, "param_groups": param_groups}

    def load_optimizer_state_dict(self, sd):
        """Accepts the torch layout above (a reference checkpoint's ``optimizer``) or this package's round-1 flat ``{"m","v"}``
        blob; anything else raises (the reference's ``optimizer.load_state_dict`` would, :302)."""
        if not isinstance(sd, dict):
            raise ValueError(f"optimizer state must be a dict, got {type(sd).__name__}")
        if "m" in sd and "v" in sd:
            if sd["m"].numel() != self.m.numel() or sd["v"].numel() != self.v.numel():
                raise ValueError("optimizer state: flat m/v size does not match this model")
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
            self._opt_step_loaded = int(sd["step"]) if "step" in sd else None
            return
        if "state" not in sd or "param_groups" not in sd:
            raise ValueError(f"optimizer state: unknown layout (keys {sorted(sd)[:6]})")
        groups = self._optimizer_names()
        pg = sd["param_groups"]
        if len(pg) != 2 or any(len(g["params"]) != len(e) for g, e in zip(pg, groups)):
            raise ValueError("optimizer state: parameter groups do not match this model "
                             f"(expected sizes {[len(e) for e in groups]}, got {[len(g['params']) for g in pg]})")
        self.m.zero_()
        self.v.zero_()
        steps = set()
        index = {}
        for g, entries in zip(pg, groups):
            for pid, e in zip(g["params"], entries):
                index[pid] = e
        for pid, st in sd["state"].items():
            if pid not in index:
                raise ValueError(f"optimizer state: unknown parameter index {pid}")
            name, ti, n = index[pid]
            if ti is None:
                continue                                  # BERT pooler: never has a gradient on this path
            for key, buf in (("exp_avg", self.m), ("exp_avg_sq", self.v)):
                t = st[key]
                dst = self._slice(buf, ti, n)
                if tuple(t.shape) != tuple(dst.shape):
                    raise ValueError(f"optimizer state: {name}.{key} has shape {tuple(t.shape)}, expected {tuple(dst.shape)}")
                dst.copy_(t.to(torch.float32))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError(f"optimizer state: per-parameter step counts differ ({sorted(steps)[:4]}...): one fused step counter here")
        self._opt_step_loaded = steps.pop() if steps else None

    def _arithmetic(self):
        """What identifies the arithmetic of a step (``resume_state``): an exact resume under another mode would not be one."""
        a = {"amp": "fp16" if self.amp16 else "bf16", "share_weights": bool(self.model.share_weights), "n_towers": len(self.model.towers())}
        if self.cosine:           # a dot-product trainer's resume_state has today's fields, no more
            a["score"] = self.score_state()
        return a

    def score_state(self):
        """The checkpoint's top-level ``score`` key of a cosine trainer (None for the dot product: no key): what the programs that build a model
        from ``--resume`` read (retriever.retrieval_utils.cosine_of)."""
        return {"kind": "cosine", "scale": self.cosine_scale, "eps": ops.COSINE_EPS} if self.cosine else None

    def resume_state(self):
        """What the reference's checkpoint keys do not carry and an exact resume needs (``load_state_dict(exact=True)``): plain CPU tensors and
        Python scalars.  Reads the loss-scale block back from the device: checkpoint time only, like `skipped_steps`."""
        scale = self._scale_state.detach().cpu().clone() if self._scale_state is not None else None
        return {"version": RESUME_VERSION, "step_seeds": [int(t.step_seed) for t in self.model.towers()], "loss_scale": scale,
                "skipped_steps": int(scale[3].item()) if scale is not None else 0, "adam_step": int(self.adam_step),
                "global_step": int(self.global_step), **self._arithmetic()}

    def _checked_resume_state(self, ckpt):
        """``ckpt["resume_state"]`` if this trainer can continue from it bit for bit; ValueError naming the field otherwise."""
        rs = ckpt.get("resume_state")
        if not isinstance(rs, dict):
            raise ValueError("exact resume: the checkpoint has no 'resume_state' (written by the reference or by an earlier version of this "
                             "package): load it with exact=False / without --resume_exact")
        if rs.get("version") != RESUME_VERSION:
            raise ValueError(f"exact resume: resume_state 'version' is {rs.get('version')!r}, this package reads version {RESUME_VERSION}")
        for field, mine in {"score": None, **self._arithmetic()}.items():        # 'score' is absent on both sides of a dot-product resume
            if rs.get(field) != mine:
                raise ValueError(f"exact resume: '{field}' was {rs.get(field)!r} when the checkpoint was written and is {mine!r} in this trainer"
                                 + (" (CLDRD_AMP)" if field == "amp" else ""))
        for field in ("step_seeds", "loss_scale", "skipped_steps", "adam_step", "global_step"):
            if field not in rs:
                raise ValueError(f"exact resume: resume_state has no '{field}'")
        scale = rs["loss_scale"]
        if self._scale_state is not None and (not isinstance(scale, torch.Tensor) or tuple(scale.shape) != tuple(self._scale_state.shape)):
            raise ValueError(f"exact resume: 'loss_scale' must be the float[{self._scale_state.numel()}] loss-scale block")
        if len(rs["step_seeds"]) != len(self.model.towers()):
            raise ValueError("exact resume: 'step_seeds' must hold one dropout step counter per tower")
        if int(rs["skipped_steps"]) != (int(scale[3].item()) if self._scale_state is not None else 0):
            raise ValueError("exact resume: 'skipped_steps' disagrees with the skipped count of the 'loss_scale' block")
        return rs

    def state_dict(self):
        """Checkpoint payload in the reference's shape (nway_listwise_1.py:418-426): DDP-style ``module.`` prefixed keys, the
        optimizer in torch's ``state_dict()`` layout, the scheduler as ``LambdaLR.state_dict()`` would give it; plus ONE key the reference does
        not know and, loading by name, ignores: ``resume_state`` (`resume_state`)."""
        return {"global_step": self.global_step,
                "state_dict": {"module." + k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                "optimizer": self.optimizer_state_dict(),
                "scheduler": {"base_lrs": [self.lr0, self.lr0], "last_epoch": self.global_step, "_step_count": self.global_step + 1,
                              "_get_lr_called_within_step": False, "_last_lr": [self.lr(), self.lr()], "lr_lambdas": [None, None],
                              "warmup_steps": self.warmup_steps, "total_steps": self.total_steps},
                "resume_state": self.resume_state(), **({"score": self.score_state()} if self.cosine else {})}

    def load_state_dict(self, ckpt, exact=False):
        """``exact=False``: parameters, moments and the step counters, as the reference's ``--resume`` (``resume_state`` is ignored): the dropout
        step counters and the loss-scale block stay as they are, Adam's step is the loaded one, which already excludes skipped steps.

        ``exact=True``: after that, everything else a step depends on is put back from ``resume_state`` - every tower's dropout step counter,
        the whole loss-scale block (copied INTO the tensor: a captured graph holds its address), ``adam_step`` and ``global_step`` as the saving
        trainer held them.  ``adam_step`` then counts the skipped steps again and the block's skipped count is back, so the bias-correction
        exponent (their difference), ``skipped_steps()`` and the ``step`` of later checkpoints are those of the run that was never interrupted.
        ValueError (nothing loaded) when the checkpoint has no ``resume_state``, an unknown ``version``, or another arithmetic mode
        (CLDRD_AMP), ``share_weights`` or tower count than this trainer.
        The capture policy is no part of the state: a fresh trainer runs its eager warm-up steps and captures again, and with
        ``deterministic=True`` an eager step equals a replayed one bit for bit (tests/test_gpu_deterministic.py), so the warm-up does not
        show in the results; a trainer that has captured already keeps replaying.  Bit equality with the uninterrupted run needs
        ``deterministic=True`` on both sides (float atomics otherwise) and holds for one process."""
        rs = self._checked_resume_state(ckpt) if exact else None
        sd = {k[7:] if k.startswith("module.") else k: v for k, v in ckpt["state_dict"].items()}
        self.model.load_state_dict(sd)
        self._opt_step_loaded = None
        if "optimizer" in ckpt:
            self.load_optimizer_state_dict(ckpt["optimizer"])
        self.global_step = int(ckpt.get("global_step", 0))
        if "scheduler" in ckpt and isinstance(ckpt["scheduler"], dict) and "last_epoch" in ckpt["scheduler"] and "global_step" not in ckpt:
            self.global_step = int(ckpt["scheduler"]["last_epoch"])
        self.adam_step = self.global_step if self._opt_step_loaded is None else self._opt_step_loaded
        if self._scale_state is not None:
            self._scale_state[3] = 0.0          # the loaded step already excludes the skipped ones
        if rs is not None:
            self.global_step, self.adam_step = int(rs["global_step"]), int(rs["adam_step"])
            if self._scale_state is not None:
                self._scale_state.copy_(rs["loss_scale"])
            for t, s in zip(self.model.towers(), rs["step_seeds"]):
                t.step_seed = int(s)
        for t in self.model.towers():
            t.refresh_shadows(need_transposed=True)


# =================================================================================================================
# Command line of reference trainer/multistep-curriculum/nway_listwise_{1,2,3}.py (flags, defaults, log and checkpoint
# formats), plus: --loss (the reference hard-codes lambda_mrr), --token_cache_dir (tokenise once) and
# --synthetic_steps (run on generated MSMARCO-shaped batches when no dataset / tokenizer is at hand).
# =================================================================================================================
def get_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="N-way listwise distillation training on MI355X (CL-DRD multistep curriculum)")
    ap.add_argument("--queries_path", default=None)
    ap.add_argument("--collection_path", default=None)
    ap.add_argument("--training_path", default=None)
    ap.add_argument("--experiment_folder", default="experiments/multistep-curriculum/")
    ap.add_argument("--model_name_or_path", default="sebastian-hofstaetter/distilbert-dot-tas_b-b256-msmarco")
    ap.add_argument("--tokenizer_name_or_path", default="distilbert-base-uncased")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--resume_exact", action="store_true", default=False,
                    help="with --resume: go on where the checkpoint was written - dropout seeds, loss-scale state and the position in the epoch's "
                         "data from its resume_state - instead of restarting the epoch as the reference does (README: Resuming a run)")
    ap.add_argument("--model_checkpoint", default=None)
    ap.add_argument("--seed", default=4680, type=int)
    ap.add_argument("--show_progress", default=True, type=bool)
    ap.add_argument("--run_folder", default="experiment")
    ap.add_argument("--log_dir", default="log/")
    ap.add_argument("--logging_steps", default=50, type=int)
    ap.add_argument("--evaluate_steps", default=10000, type=int)
    ap.add_argument("--model_save_dir", default="models")
    ap.add_argument("--learning_rate", default=7e-6, type=float)
    ap.add_argument("--weight_decay", default=0.01, type=float)
    ap.add_argument("--adam_epsilon", default=1e-8, type=float)
    ap.add_argument("--max_grad_norm", default=1.0, type=float)
    ap.add_argument("--num_train_epochs", default=4, type=int)
    ap.add_argument("--warmup_steps", default=4000, type=int)
    ap.add_argument("--reg_lambda", default=0.0, type=float)
    ap.add_argument("--query_max_len", default=30, type=int)
    ap.add_argument("--passage_max_len", default=256, type=int)
    ap.add_argument("--use_fp16", default=True, type=bool, help="accepted for compatibility: MFMA operands are fp16 (loss-scaled backward) with fp32 master weights; CLDRD_AMP=bf16 selects the "
                    "all-bf16 mode (every operand bf16, no loss scale)")
    ap.add_argument("--train_batch_size", default=8, type=int)
    ap.add_argument("--share_weights", action="store_true", default=False)
    ap.add_argument("--label_mode", default="8", type=str)
    ap.add_argument("--in_batch_loss", action="store_true", default=False)
    ap.add_argument("--all_in_batch_neg", action="store_true", default=False)
    ap.add_argument("--n_gpu", default=1, type=int)
    ap.add_argument("--local_rank", default=-1, type=int)
    ap.add_argument("--loss", default="lambda_mrr", choices=LOSS_KINDS + CONTRASTIVE_KINDS)
    ap.add_argument("--ce_temperature", default=None, type=float,
                    help="--loss softmax_ce: the temperature the logits are divided by (default 1; it multiplies with --cosine_scale)")
    ap.add_argument("--ce_pos_min", default=None, type=float,
                    help="--loss softmax_ce: columns with label >= this are positives (default: the columns at the row's maximum label)")
    ap.add_argument("--ce_neg_max", default=None, type=float,
                    help="--loss softmax_ce: columns with label <= this (and not positive) are negatives, the rest is left out (default 0)")
    ap.add_argument("--ce_mask_duplicate_pids", action="store_true", default=False,
                    help="--loss softmax_ce: a negative column whose passage id is also behind a positive or left-out column of its row is left out")
    ap.add_argument("--weighing_scheme", default=None, choices=WEIGHING_SCHEMES,
                    help="--loss lambda_loss: the pair weights (reference losses/standard_lambda_rank.py:98-127; default none: every pair 1)")
    ap.add_argument("--lambda_k", default=None, type=int, help="--loss lambda_loss: rank truncation k (default 0: none)")
    ap.add_argument("--lambda_sigma", default=None, type=float, help="--loss lambda_loss: score-difference weight (default 1)")
    ap.add_argument("--lambda_mu", default=None, type=float, help="--loss lambda_loss: mu of ndcgLoss2PP_scheme (default 10)")
    ap.add_argument("--lambda_gain", default=None, choices=("power", "linear"), help="--loss lambda_loss: gain 2^label - 1 | label - 1 (default power)")
    ap.add_argument("--lambda_log", default=None, choices=("natural", "binary"), help="--loss lambda_loss: logarithm of the loss (default natural)")
    ap.add_argument("--label_source", default="rank", choices=LABEL_SOURCES,
                    help="labels of --loss lambda_loss: the label-mode constants (rank) or the teacher scores of the training file "
                         "(teacher; dataset.curriculum_file --with_scores)")
    ap.add_argument("--neg_score_mode", default=None, choices=NEG_SCORE_MODES,
                    help="--label_source teacher: every negative keeps its own teacher score (original, the default) or gets the mean over the negatives")
    ap.add_argument("--teacher_label_shift", default=None, choices=LABEL_SHIFTS,
                    help="--label_source teacher: row_min subtracts the row's lowest score first (scores <= 0, such as log-softmax outputs, would "
                         "otherwise all clamp to label 0); default none")
    ap.add_argument("--distill_loss", default=None, choices=DISTILL_KINDS,
                    help="add distill_alpha * KLDiv(distill_T) / MarginMSE of the logits against the teacher scores of the training file "
                         "(dataset.curriculum_file --with_scores) to --loss")
    ap.add_argument("--distill_alpha", default=1.0, type=float, help="weight of the --distill_loss term")
    ap.add_argument("--distill_T", default=1.0, type=float, help="temperature of --distill_loss kl_div")
    ap.add_argument("--distill_only", action="store_true", default=False, help="drop the --loss term: total = distill_alpha * distill loss")
    ap.add_argument("--apply_consine_similarity", "--apply_cosine_similarity", dest="apply_consine_similarity", action="store_true", default=False,
                    help="score with cosine_scale * cosine similarity instead of the dot product (the reference's spelling, "
                         "scripts/unity/cosine_nway_listwise.sh; README: Cosine-similarity scoring)")
    ap.add_argument("--cosine_scale", default=None, type=float, help="--apply_consine_similarity: the factor on the cosine (default 1)")
    ap.add_argument("--deterministic", action="store_true", default=False,
                    help="bit-reproducible steps: embedding-table gradients as fixed-order per-row sums instead of float atomics (README: cost)")
    ap.add_argument("--tas_clusters", default=None,
                    help="topic-aware batches: the qid<TAB>cluster file of dataset.query_clusters; every batch is drawn from one cluster "
                         "where the cluster sizes allow (README: Topic-aware batches)")
    ap.add_argument("--token_cache_dir", default=None)
    ap.add_argument("--loader_workers", default=4, type=int, help="collate (tokenise / gather from the token cache) worker processes; "
                    "batches arrive in pinned memory, a few steps ahead of the GPU")
    ap.add_argument("--synthetic_steps", default=0, type=int, help="steps per epoch on generated batches (no dataset files needed)")
    ap.add_argument("--synthetic_nway", default=30, type=int)
    ap.add_argument("--synthetic_fixed", action="store_true", default=False, help="every synthetic passage passage_max_len tokens long (default: MS MARCO-shaped lengths)")
    ap.add_argument("--synthetic_model", default="distilbert", choices=("distilbert", "tiny"),
                    help="random-init architecture for --synthetic_steps runs without a model directory (tiny: encoder.tiny_config)")
    # validation while training (the reference scripts' names, scripts/unity/*.sh): at every checkpoint rank 0 re-ranks the dev run with the student
    ap.add_argument("--dev_path", default=None, help="dev run file (qid pid [rank] [score]) the student re-ranks at every evaluate_steps")
    ap.add_argument("--dev_queries_path", default=None)
    ap.add_argument("--dev_qrels_path", default=None)
    ap.add_argument("--dev_top_k", default=0, type=int, help="candidates per dev query, in run order (0: all)")
    ap.add_argument("--dev_batch_size", default=512, type=int, help="sequences per encoder batch of a validation")
    ap.add_argument("--dev_qrels_trec", action="store_true", default=False, help="--dev_qrels_path is space separated (TREC)")
    args = ap.parse_args(argv)
    if args.resume_exact and not args.resume:
        ap.error("--resume_exact needs --resume CKPT")
    dev_flags = [args.dev_path, args.dev_queries_path, args.dev_qrels_path]
    if any(v is not None for v in dev_flags) and not all(v is not None for v in dev_flags):
        ap.error("--dev_path, --dev_queries_path and --dev_qrels_path go together: all three or none")
    if args.dev_path is not None and args.synthetic_steps > 0:
        ap.error("--dev_path needs --collection_path for the passage texts; --synthetic_steps runs have no collection file")
    if args.dev_path is not None and (args.dev_batch_size < 1 or args.dev_top_k < 0):
        ap.error("--dev_batch_size must be >= 1 and --dev_top_k >= 0")
    if args.cosine_scale is not None and not args.apply_consine_similarity:
        ap.error("--cosine_scale is an option of --apply_consine_similarity; it was given without it")
    if args.cosine_scale is not None and not (math.isfinite(args.cosine_scale) and args.cosine_scale > 0.0):
        ap.error("--cosine_scale must be finite and > 0")
    if args.distill_loss is None and args.distill_only:
        ap.error("--distill_only needs --distill_loss")
    if args.distill_loss is not None and args.label_mode == "1" and args.synthetic_steps <= 0:
        ap.error("--distill_loss needs a relT / most-hard / semi-hard training file with scores; --label_mode 1 files have none")
    if args.distill_loss is not None and (not args.distill_alpha >= 0.0 or not args.distill_T > 0.0):
        ap.error("--distill_alpha must be >= 0 and --distill_T > 0")
    defaults = {**LAMBDA_DEFAULTS, **TEACHER_LABEL_DEFAULTS}
    check_loss_options(args.loss, args.label_source, args.in_batch_loss, args.label_mode, args.synthetic_steps > 0,
                       given=[k_ for k_ in defaults if getattr(args, k_) is not None],           # a ValueError that names the flag
                       **_ce_options(args))
    if args.ce_mask_duplicate_pids and args.synthetic_steps > 0:
        raise ValueError("--ce_mask_duplicate_pids needs the passage ids of a training file (batch['nway_pids']); --synthetic_steps batches have none")
    if args.tas_clusters is not None and args.synthetic_steps > 0:
        raise ValueError("--tas_clusters groups the queries of a training file by cluster; --synthetic_steps batches are generated whole and have none")
    if args.lambda_k is not None and args.lambda_k < 0 or args.lambda_sigma is not None and not args.lambda_sigma > 0.0:
        raise ValueError("--lambda_k must be >= 0 (0: no truncation) and --lambda_sigma > 0")
    args.run_folder = os.path.join(args.experiment_folder, args.run_folder)
    args.log_dir = os.path.join(args.run_folder, args.log_dir)
    args.model_save_dir = os.path.join(args.run_folder, args.model_save_dir)
    return args


def _ce_options(args):
    """The --ce_* flags as the keyword arguments of check_loss_options / NwayTrainer (None / False: not given)."""
    return {"ce_temperature": getattr(args, "ce_temperature", None), "ce_pos_min": getattr(args, "ce_pos_min", None),
            "ce_neg_max": getattr(args, "ce_neg_max", None), "ce_mask_duplicate_pids": bool(getattr(args, "ce_mask_duplicate_pids", False))}


def set_env(args):
    """One process per GPU: ranks come from torchrun's environment (or --local_rank as in the reference, :40-49)."""
    if args.local_rank == -1 and "LOCAL_RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        args.local_rank = int(os.environ["LOCAL_RANK"])
    if args.local_rank != -1:
        torch.cuda.set_device(args.local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl")
        args.nranks = dist.get_world_size()
        args.distributed = args.nranks > 1
    else:
        args.nranks, args.distributed = 1, False
    args.device = torch.device("cuda", max(args.local_rank, 0))
    args.rank = dist.get_rank() if args.distributed else 0
    cap_host_threads()
    return args


def write_train_logs(epoch, step, loss_val, mrr_val, recall_val, lr, filename, cutoff=10, **kwargs):
    """Tab-separated log of reference :78-90 (including its quirk: the first call only writes the header)."""
    if not os.path.exists(filename):
        with open(filename, "w") as fh:
            fh.write("\t".join(["epoch", "step", "loss_val", f"mrr@{cutoff}", f"recall@{cutoff}", "lr"] + list(kwargs)) + "\n")
    else:
        with open(filename, "a") as fh:
            fh.write(f"{epoch}\t{step}\t{loss_val:.3f}\t{mrr_val:.3f}\t{recall_val:.3f}\t{lr:.10f}")
            for v in kwargs.values():
                fh.write(f"\t{v:.3f}")
            fh.write("\n")


class _Avg:
    def __init__(self):
        self.reset()

    def reset(self):
        self.sum, self.n = 0.0, 0

    def update(self, v):
        self.sum += float(v)
        self.n += 1

    @property
    def avg(self):
        return self.sum / max(self.n, 1)


class _EpochPosition(torch.utils.data.Sampler):
    """The index stream of a training loader (a batch sampler, or the plain sampler of a ``batch_size=None`` loader), handed on unchanged,
    with the two things an exact resume needs from it:

    ``epoch_state``: the state of the loader's ``torch.Generator`` at the moment the current epoch's stream was started, that is right
    before the sampler under it draws the epoch's permutation (None without a generator).  A state, not a count of draws, and taken HERE and
    not around ``iter(loader)``: the DataLoader draws a worker seed of its own from the same generator whenever it builds an iterator - every
    epoch without workers, once in its life with persistent ones - so a resumed epoch (always a new iterator) would meet the generator one
    draw further than the epoch it continues.  From this point on the draws are the sampler's alone.

    ``resume(skip, state)``: the NEXT stream that is started first puts ``state`` back into the generator and then passes over its first
    ``skip`` items: index batches that are never fetched, tokenised or collated.  Streams after it are untouched.  (A stream counts as
    started at its first item: the DataLoader makes iterators it never reads from.)"""

    def __init__(self, inner, generator=None):
        self.inner, self.generator = inner, generator
        self.epoch_state = None
        self._pending = None

    def resume(self, skip, state):
        self._pending = (int(skip), state)

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        (skip, state), self._pending = self._pending or (0, None), None
        if self.generator is not None:
            if state is not None:
                self.generator.set_state(state)
            self.epoch_state = self.generator.get_state()
        for i, item in enumerate(self.inner):
            if i >= skip:
                yield item


def read_query_clusters(path):
    """The ``qid<TAB>cluster`` file of dataset.query_clusters -> ({qid: cluster}, 16-hex digest of the file's bytes).  ValueError naming
    --tas_clusters and the line for anything else than two integer fields with cluster >= 0."""
    import hashlib
    with open(path, "rb") as fh:
        data = fh.read()
    out = {}
    for no, line in enumerate(data.decode("utf-8", errors="replace").splitlines(), start=1):
        a = line.split("\t")
        try:
            if len(a) != 2:
                raise ValueError
            qid, c = int(a[0]), int(a[1])
            if c < 0:
                raise ValueError
        except ValueError:
            raise ValueError(f"--tas_clusters: line {no} of {path} is not 'qid<TAB>cluster' (two integers, cluster >= 0): {line[:80]!r}") from None
        out[qid] = c
    if not out:
        raise ValueError(f"--tas_clusters: {path} holds no line")
    return out, hashlib.sha256(data).hexdigest()[:16]


class TopicBatchSampler(torch.utils.data.Sampler):
    """Topic-aware batches (TAS, Hofstaetter et al. 2021): the batch sampler of --tas_clusters.  One epoch, every draw taken from
    ``generator``:

      1. ``perm = randperm(len(dataset))``;
      2. ``perm`` grouped stably by the cluster of ``dataset.train_examples[i]["qid"]``;
      3. each cluster's list cut into full batches of ``batch_size`` (PURE batches: one cluster);
      4. the clusters' remainders, concatenated in ascending cluster order, cut into batches of ``batch_size`` (MIXED batches); a final
         remainder shorter than a batch is dropped, as ``drop_last`` drops it;
      5. all batches yielded in the order ``randperm(n_batches)``.

    Exactly ``len(dataset) // batch_size`` batches and no example twice: the epoch length, the schedule and the resume position keep the
    values they have under the RandomSampler.  Which batches are pure is decided by the cluster sizes alone, not by the draws."""

    def __init__(self, dataset, cluster_of_qid, batch_size, generator=None):
        self.batch_size, self.generator = int(batch_size), generator
        if self.batch_size < 1:
            raise ValueError("TopicBatchSampler: batch_size must be >= 1")
        qids = [int(ex["qid"]) for ex in dataset.train_examples]
        missing = [q for q in qids if q not in cluster_of_qid]
        if missing:
            raise ValueError(f"--tas_clusters: {len(missing)} of the {len(qids)} training examples have a qid the cluster file does not name "
                             f"(the first: {missing[0]}); cluster the queries of this training file (dataset.query_clusters --training_path)")
        self.cluster = torch.tensor([cluster_of_qid[q] for q in qids], dtype=torch.int64)
        self.sizes = torch.bincount(self.cluster) if len(qids) else torch.zeros(0, dtype=torch.int64)
        self.n_pure = int((self.sizes // self.batch_size).sum())
        self.n_batches = len(qids) // self.batch_size

    def with_generator(self, generator):
        """the same sampler drawing from another generator (replayed_epoch_state)"""
        other = copy.copy(self)
        other.generator = generator
        return other

    def describe(self):
        n = int(self.cluster.numel())
        share = self.n_pure * self.batch_size / n if n else 0.0
        return (f"--tas_clusters: {self.n_pure} pure + {self.n_batches - self.n_pure} mixed batches of {self.batch_size} per epoch over "
                f"{int((self.sizes > 0).sum())} clusters; {100.0 * share:.1f} % of the examples are in pure batches")

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        B, n = self.batch_size, int(self.cluster.numel())
        perm = torch.randperm(n, generator=self.generator)
        grouped = perm[torch.sort(self.cluster[perm], stable=True).indices]
        pure, rest, start = [], [], 0
        for m in self.sizes.tolist():
            full = m - m % B
            pure.append(grouped[start:start + full])
            rest.append(grouped[start + full:start + m])
            start += m
        rest = torch.cat(rest) if rest else grouped[:0]
        rows = torch.cat(pure + [rest[:rest.numel() - rest.numel() % B]]).view(-1, B) if n >= B else grouped[:0].view(0, B)
        assert rows.shape[0] == self.n_batches
        for b in torch.randperm(self.n_batches, generator=self.generator).tolist():
            yield rows[b].tolist()


def _position_of(loader) -> _EpochPosition:
    return loader.batch_sampler if loader.batch_sampler is not None else loader.sampler


def replayed_epoch_state(loader, seed, epochs):
    """``epoch_state`` of epoch ``epochs`` (zero-based) of ``loader`` as a generator seeded ``seed`` reaches it: what a rank other than 0 puts
    in the place of the checkpoint's state, which is rank 0's.  Replays the draws of the completed epochs without fetching anything: the
    DataLoader's worker seed where it builds an iterator (see `_EpochPosition`), then one pass over a sampler that draws what the one in
    use draws: a `TopicBatchSampler` on the replay's generator under --tas_clusters, a RandomSampler otherwise."""
    pos = _position_of(loader)
    if pos.generator is None:
        return None
    g = torch.Generator()
    g.manual_seed(seed)
    sampler = pos.inner.with_generator(g) if isinstance(pos.inner, TopicBatchSampler) else torch.utils.data.RandomSampler(loader.dataset, generator=g)
    keeps_iterator = loader.persistent_workers and loader.num_workers > 0
    for e in range(epochs + 1):
        if e == 0 or not keeps_iterator:
            torch.empty((), dtype=torch.int64).random_(generator=g)
        if e < epochs:
            for _ in sampler:
                pass
    return g.get_state()


def check_resume_position(saved, current):
    """``--resume_exact``: the position (epoch, step_in_epoch) of a checkpoint means the same batches only under the values it was written
    with.  ValueError naming the first of POSITION_FIELDS that differs, with both values."""
    for field in POSITION_FIELDS:
        if field not in saved:
            raise ValueError(f"--resume_exact: the checkpoint's resume_state has no '{field}' (it was not written by the training command line)")
        if saved[field] != current[field]:
            raise ValueError(f"--resume_exact: {field} was {saved[field]} when the checkpoint was written and is {current[field]} now")
    for field in TAS_POSITION_FIELDS:          # absent on both sides without --tas_clusters
        if saved.get(field) != current.get(field):
            raise ValueError(f"--resume_exact: {field} was {saved.get(field)!r} when the checkpoint was written and is {current.get(field)!r} now "
                             "(--tas_clusters: the batches of an epoch depend on the cluster file)")


def save_checkpoint(ckpt, path):
    """``torch.save`` under a temporary name in the same directory, then ``os.replace``: a job killed during the write leaves no truncated file
    under the name a restart would pick."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def build_dataloader(args):
    """Label mode -> file constructor as reference :173-245; per-rank batch = train_batch_size // nranks, shuffle, drop_last."""
    from transformers import AutoTokenizer
    from ..dataset.nway_dataset import NwayDataset
    check_loss_options(getattr(args, "loss", "lambda_mrr"), getattr(args, "label_source", "rank"), getattr(args, "in_batch_loss", False),
                       label_mode=args.label_mode, **_ce_options(args))      # before anything is loaded
    tas = getattr(args, "tas_clusters", None)
    cluster_of_qid, tas_digest = read_query_clusters(tas) if tas else (None, None)          # a malformed file is refused before the tokenizer is loaded
    tok = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path)
    a = (args.queries_path, args.collection_path, args.training_path, tok)
    kw = dict(max_query_len=args.query_max_len, max_passage_len=args.passage_max_len, label_mode=args.label_mode)
    shard = dict(rank=args.rank, nranks=args.nranks) if args.distributed else {}
    mode = args.label_mode
    distill = getattr(args, "distill_loss", None) is not None
    if distill and mode == "1":
        raise ValueError("--distill_loss: label mode 1 files ({qid, rel_pid, neg_pids}) carry no teacher scores")
    if distill or getattr(args, "label_source", "rank") == "teacher":
        shard["teacher_scores"] = True
    if mode == "1":
        if args.distributed:
            raise NotImplementedError
        ds = NwayDataset.create_from_json_line_file(*a, **kw)
    elif mode in ("2", "4"):
        ds = NwayDataset.create_from_relT_most_semi_hard_file(*a, **kw, **shard)
    elif mode in ("3", "9"):
        ds = NwayDataset.create_from_10relT_20neg_file(*a, **kw, **shard)
    elif mode in ("5", "10"):
        ds = NwayDataset.create_from_20relT_10neg_file(*a, **kw, **shard)
    elif mode == "6":
        ds = NwayDataset.create_from_30relT_file(*a, **kw, **shard)
    elif mode in ("7", "8"):
        ds = NwayDataset.create_from_5relT_25neg_file(*a, **kw, **shard)
    else:
        raise ValueError(f"label mode {mode} not implemented")
    if args.token_cache_dir:
        # every rank holds the full query / passage tables, so the cache is the same everywhere: rank 0 builds and writes it
        # (atomic renames), the others load it after the barrier instead of racing on the same files
        if args.distributed:
            if args.rank == 0:
                ds.with_token_cache(args.token_cache_dir)
            dist.barrier()
            if args.rank != 0:
                ds.with_token_cache(args.token_cache_dir, build=False)
        else:
            ds.with_token_cache(args.token_cache_dir)
    assert args.train_batch_size % args.nranks == 0
    g = torch.Generator()
    g.manual_seed(args.seed + args.rank)
    nw = max(int(getattr(args, "loader_workers", 1)), 0)
    # shuffle=True, drop_last=True spelled out as the samplers the DataLoader would build from them (same generator, same draws, same
    # batches), so that the batch sampler can be the one that knows its position (`_EpochPosition`, --resume_exact)
    U = torch.utils.data
    if cluster_of_qid is not None:
        batches = TopicBatchSampler(ds, cluster_of_qid, args.train_batch_size // args.nranks, generator=g)
        batches.file_digest = tas_digest          # of the file's bytes: a position field of the checkpoints (train)
        if args.rank == 0:
            sys.stderr.write(batches.describe() + "\n")
    else:
        batches = U.BatchSampler(U.RandomSampler(ds, generator=g), args.train_batch_size // args.nranks, drop_last=True)
    return ds, U.DataLoader(ds, batch_sampler=_EpochPosition(batches, g), num_workers=nw, collate_fn=ds.collate_fn, generator=g, pin_memory=True,
                            **(dict(prefetch_factor=4, persistent_workers=True) if nw else {}))


class _SyntheticBatches(torch.utils.data.Dataset):
    """``--synthetic_steps`` batches of the collate_fn layout from the portable generator (synthetic.nway_batch): item i IS batch i (a
    function of (seed, rank, i) only), so the loader below hands them out with ``batch_size=None`` from worker processes, pinned, like the
    real one."""

    def __init__(self, args):
        self.args = args

    def __len__(self):
        return self.args.synthetic_steps

    def __getitem__(self, i):
        from .. import synthetic as syn
        a = self.args
        b = syn.nway_batch(a.seed + 1000 * a.rank + i, a.train_batch_size // a.nranks, a.synthetic_nway, a.query_max_len,
                           a.passage_max_len, vocab=getattr(a, "synthetic_vocab", syn.VOCAB), ragged=not getattr(a, "synthetic_fixed", False),
                           label_kind="teacher" if a.loss in ("kl_div", "margin_mse") else "mode9",
                           with_teacher_scores=getattr(a, "distill_loss", None) is not None or getattr(a, "label_source", "rank") == "teacher")
        return attach_lengths(b)


def _synthetic_loader(args):
    nw = max(int(getattr(args, "loader_workers", 1)), 0)
    ds = _SyntheticBatches(args)
    # item i is batch i: the sequential sampler (what shuffle=False builds) under the position wrapper skips whole batches by index
    return torch.utils.data.DataLoader(ds, batch_size=None, sampler=_EpochPosition(torch.utils.data.SequentialSampler(ds)), num_workers=nw,
                                       pin_memory=True, **(dict(prefetch_factor=4, persistent_workers=True) if nw else {}))


def common_steps_per_epoch(local_steps: int, distributed: bool, dev=None, group=None) -> int:
    """Examples are sharded ``line_idx % nranks`` with ``drop_last`` (reference dataset/nway_dataset.py:305), so ranks can differ by
    one batch per epoch; every rank runs MIN over ranks steps: same schedule length (t_total) everywhere and no rank left alone in
    a gradient all-reduce at the end of an epoch."""
    if not distributed:
        return int(local_steps)
    t = torch.tensor([int(local_steps)], dtype=torch.int64, device=dev if dist.get_backend(group) == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
    return int(t.item())


def batch_to_device(batch, dev):
    """Move a collated batch to the device (asynchronously when the loader pinned it); "lengths" stay on the host."""
    batch = attach_lengths(batch)
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(dev, non_blocking=True)
        elif hasattr(v, "items"):
            out[k] = {kk: (vv.to(dev, non_blocking=True) if (isinstance(vv, torch.Tensor) and kk != "lengths") else vv) for kk, vv in v.items()}
        else:
            out[k] = v
    return out


class _DevValidation:
    """``--dev_path`` / ``--dev_queries_path`` / ``--dev_qrels_path`` of a training run (rank 0): the dev pool built once, then one
    ``NwayTrainer.validate`` per saved checkpoint - a line of ``<log_dir>/dev_logs.log`` and ``<run_folder>/dev_best.json`` rewritten."""

    def __init__(self, args):
        from transformers import AutoTokenizer
        from ..evaluation import DevPool, RerankingEvaluator
        tok = AutoTokenizer.from_pretrained(args.tokenizer_name_or_path)
        self.pool = DevPool(args.dev_path, args.dev_queries_path, args.collection_path, tok, args.query_max_len, args.passage_max_len,
                            top_k=args.dev_top_k, token_cache_dir=args.token_cache_dir)
        self.evaluator = RerankingEvaluator(args.dev_qrels_path, is_trec=args.dev_qrels_trec)
        self.batch_size = args.dev_batch_size
        self.log_file = os.path.join(args.log_dir, "dev_logs.log")
        self.best_file = os.path.join(args.run_folder, "dev_best.json")
        self.best = None
        if args.resume and os.path.exists(self.best_file):        # a resumed run goes on from the best it had
            import json
            with open(self.best_file) as fh:
                self.best = json.load(fh)

    def validate(self, trainer, epoch, ckpt_path):
        import time
        from ..evaluation.reranking_evaluator import update_dev_best, write_dev_logs
        t0 = time.perf_counter()
        metrics = trainer.validate(self.pool, self.evaluator, batch_size=self.batch_size)
        write_dev_logs(self.log_file, epoch, trainer.global_step, metrics, time.perf_counter() - t0)
        self.best = update_dev_best(self.best_file, self.best, metrics, trainer.global_step, epoch, ckpt_path)
        return metrics


def _dev_validation(args):
    return _DevValidation(args) if getattr(args, "dev_path", None) else None


def _n_rel(args):
    """The label mode's number of relT passages: where the negatives of a slate begin (--neg_score_mode mean).  Synthetic batches have
    --synthetic_nway passages whatever the label mode."""
    from ..dataset.nway_dataset import _REL
    n = _REL.get(str(getattr(args, "label_mode", None)))
    return min(n, args.synthetic_nway) if n is not None and args.synthetic_steps > 0 else n


def _cosine_kw(args):
    """NwayDualEncoder's scorer keywords from --apply_consine_similarity / --cosine_scale (none of them without the flag)."""
    if not getattr(args, "apply_consine_similarity", False):
        return {}
    scale = getattr(args, "cosine_scale", None)
    return {"cosine": True, "cosine_scale": 1.0 if scale is None else float(scale)}


def train(args):
    """Epoch / step loop of reference :328-426 on top of NwayTrainer.train_step."""
    import random
    import numpy as np
    dev = args.device
    if args.synthetic_steps > 0:
        loader, n_examples = _synthetic_loader(args), args.synthetic_steps * args.train_batch_size
    else:
        ds, loader = build_dataloader(args)
        n_examples = len(ds)
    if args.synthetic_steps > 0 and not os.path.isdir(str(args.model_name_or_path)):
        from ..encoder import EncoderConfig
        if args.synthetic_model == "tiny":
            from ..encoder import tiny_config
            cfg = tiny_config()
        else:
            cfg = EncoderConfig(arch="distilbert")
        args.synthetic_vocab = cfg.vocab_size
        model = NwayDualEncoder(cfg, share_weights=args.share_weights, in_batch_loss=args.in_batch_loss,
                                all_in_batch_neg=args.all_in_batch_neg, **_cosine_kw(args))
    else:
        model = NwayDualEncoder(args.model_name_or_path, share_weights=args.share_weights, in_batch_loss=args.in_batch_loss,
                                all_in_batch_neg=args.all_in_batch_neg, **_cosine_kw(args))
    model.to(dev)
    model.train()
    steps_per_epoch = common_steps_per_epoch(len(loader), args.distributed, dev)
    t_total = steps_per_epoch * args.num_train_epochs
    trainer = NwayTrainer(model, loss=args.loss, learning_rate=args.learning_rate, weight_decay=args.weight_decay,
                          adam_epsilon=args.adam_epsilon, max_grad_norm=args.max_grad_norm, warmup_steps=args.warmup_steps,
                          total_steps=t_total, reg_lambda=args.reg_lambda, distill=getattr(args, "distill_loss", None),
                          distill_alpha=getattr(args, "distill_alpha", 1.0), distill_T=getattr(args, "distill_T", 1.0),
                          distill_only=getattr(args, "distill_only", False), deterministic=getattr(args, "deterministic", False),
                          label_source=getattr(args, "label_source", "rank"), n_rel=_n_rel(args),
                          **{k_: getattr(args, k_, None) for k_ in (*LAMBDA_DEFAULTS, *TEACHER_LABEL_DEFAULTS)}, **_ce_options(args))
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)            # after model / loader construction, as the reference does (:282)
    start_epoch, first_step = 0, 0
    position = _position_of(loader)
    # what (epoch, step_in_epoch) of a checkpoint depends on (POSITION_FIELDS): written into every checkpoint, compared by --resume_exact
    where = {"train_batch_size": args.train_batch_size, "nranks": args.nranks, "seed": args.seed, "dataset_len": len(loader.dataset),
             "steps_per_epoch": steps_per_epoch, "num_train_epochs": args.num_train_epochs}
    if getattr(args, "tas_clusters", None):
        where.update(tas_clusters=str(args.tas_clusters), tas_clusters_digest=position.inner.file_digest)
    if args.resume:
        assert args.model_checkpoint is None
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=False)
        if getattr(args, "resume_exact", False):
            # go on at (epoch, step_in_epoch): the first epoch's index stream starts from the generator state that epoch started from and
            # passes over the batches already consumed (a checkpoint of an epoch's last batch: all of them, and the loop moves on to the next
            # epoch).  The state in the checkpoint is rank 0's; any other rank replays its own generator up to that epoch.
            rs = ckpt.get("resume_state")
            if isinstance(rs, dict):            # (a checkpoint without one: load_state_dict says so)
                check_resume_position(rs, where)
            trainer.load_state_dict(ckpt, exact=True)
            start_epoch, first_step = int(rs["epoch"]), int(rs["step_in_epoch"])
            state = rs["generator_state"] if args.rank == 0 else replayed_epoch_state(loader, args.seed + args.rank, start_epoch)
            position.resume(first_step, state)
        else:
            trainer.load_state_dict(ckpt)
            start_epoch = ckpt["epoch"] - 1
    if args.model_checkpoint:
        assert args.resume is None
        ckpt = torch.load(args.model_checkpoint, map_location="cpu", weights_only=False)
        trainer.load_state_dict({"state_dict": ckpt["state_dict"]})
    main_rank = args.rank == 0
    if main_rank:
        os.makedirs(args.log_dir, exist_ok=True)
        os.makedirs(args.model_save_dir, exist_ok=True)
    dev_run = _dev_validation(args) if main_rank else None      # None without --dev_path: nothing below changes
    loss_m, mrr_m, rec_m, reg_m, ratio_m, kd_m = _Avg(), _Avg(), _Avg(), _Avg(), _Avg(), _Avg()
    topk = 10
    log_file = os.path.join(args.log_dir, "train_logs.log")
    for epoch in range(start_epoch, args.num_train_epochs):
        # (first_step > 0: the first epoch of an exact resume, whose loader passes over that many batches; the meters start empty, so the first
        # log line after a resume averages over the logging steps since the resume only)
        for step_i, batch in enumerate(loader, start=first_step if epoch == start_epoch else 0):
            if step_i >= steps_per_epoch:       # ranks whose shard is one batch longer stop with the others (no unmatched all-reduce)
                break
            batch = batch_to_device(batch, dev)
            if trainer.ce_mask_duplicate_pids:          # the one id array a step reads on the device (collate_fn: a numpy array)
                batch["nway_pids"] = torch.as_tensor(batch["nway_pids"]).to(dev, non_blocking=True)
            loss_out = trainer.train_step(batch)
            if main_rank and trainer.global_step % args.logging_steps == 0:
                # the reference reads loss / MRR back every step (:369-389); here only on logging steps (no per-step sync)
                logits = trainer.last_logits
                labels = trainer.metric_labels(batch, logits.shape[1])
                b_mrr, b_rec = trainer.train_metrics(logits, labels, topk)
                loss_val = float(loss_out[0].item())
                loss_m.update(loss_val), mrr_m.update(b_mrr), rec_m.update(b_rec)
                extra = {}
                if args.reg_lambda > 0.0 and trainer.last_reg is not None:
                    reg = float(trainer.last_reg.item())
                    reg_m.update(reg), ratio_m.update(reg / loss_val if loss_val else 0.0)
                    extra = dict(reg_loss=reg_m.avg, total_aux_ratio=ratio_m.avg)
                if trainer.distill is not None and trainer.last_kd is not None:
                    kd_m.update(float(trainer.last_kd.item()))          # the unweighted distillation term
                    extra["kd_loss"] = kd_m.avg
                if trainer.amp16:
                    extra["skipped_steps"] = float(trainer.skipped_steps())     # the loss-scale safety net (GradScaler's skipped steps)
                write_train_logs(epoch + 1, trainer.global_step, loss_m.avg, mrr_m.avg, rec_m.avg, trainer.lr(), filename=log_file,
                                 cutoff=topk, **extra)
                for m in (loss_m, mrr_m, rec_m, reg_m, ratio_m, kd_m):
                    m.reset()
            if main_rank and trainer.global_step % args.evaluate_steps == 0:
                ckpt = trainer.state_dict()
                ckpt["epoch"] = epoch + 1
                # the data position, for --resume_exact: zero-based epoch, batches of it consumed, the generator state its index stream started from
                ckpt["resume_state"].update(where, epoch=epoch, step_in_epoch=step_i + 1, generator_state=position.epoch_state)
                ckpt_path = os.path.join(args.model_save_dir, f"checkpoint_{trainer.global_step}.pth.tar")
                save_checkpoint(ckpt, ckpt_path)
                if dev_run is not None:
                    # rank 0 alone, no collective: the other ranks meet it at the next step's first all-reduce
                    dev_run.validate(trainer, epoch + 1, ckpt_path)
    if args.distributed:
        dist.barrier()
    return trainer


def main(argv=None):
    args = set_env(get_args(argv))
    if args.rank == 0:
        os.makedirs(args.run_folder, exist_ok=True)
        import yaml
        with open(os.path.join(args.run_folder, "args.yaml"), "w") as fh:
            yaml.dump({k: (str(v) if isinstance(v, torch.device) else v) for k, v in vars(args).items()}, fh)
    owns_group = args.local_rank != -1 and dist.is_initialized()
    try:
        train(args)
    finally:
        if owns_group:                      # the group set_env() created (torchrun / --local_rank): shut RCCL down in order
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
