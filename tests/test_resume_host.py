"""--resume_exact on the host: the data position of cldrd_amd.trainer.nway_listwise.  The training loader over the committed dataset
fixture (12 examples, batch 4: three batches per epoch) yields what the loader of the parent construction yields; resumed at (epoch, step)
from the generator state its position wrapper recorded, it yields the rest of that epoch and then the following epoch unchanged, without
fetching an example of a batch it passes over; the refusals name their field.  Every comparison is equality."""
import os
import sys

import numpy as np
import pytest
import torch

from cldrd_amd.trainer import nway_listwise as T

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 3                                       # batches per epoch of the fixture at --train_batch_size 4


def _args(tmp_path, workers):
    sys.path.insert(0, HERE)
    from toy_tokenizer import make_tokenizer
    fix = os.path.join(HERE, "golden", "nway_dataset_fixture")
    tokdir = os.path.join(str(tmp_path), "tok")
    if not os.path.isdir(tokdir):
        make_tokenizer().save_pretrained(tokdir)
    a = T.get_args(["--experiment_folder", str(tmp_path), "--run_folder", "run", "--queries_path", os.path.join(fix, "queries.tsv"),
                    "--collection_path", os.path.join(fix, "collection.tsv"), "--training_path", os.path.join(fix, "train_10relT_20neg.jsonl"),
                    "--label_mode", "9", "--tokenizer_name_or_path", tokdir, "--query_max_len", "6", "--passage_max_len", "16",
                    "--train_batch_size", "4", "--loader_workers", str(workers)])
    a.rank, a.nranks, a.distributed = 0, 1, False
    return a


def _qids(batch):
    return tuple(np.asarray(batch["qid"]).tolist())


def _run_epochs(loader, epochs):
    """-> ([epoch][batch] qid tuples, [epoch] generator state the position wrapper recorded for it)"""
    pos = T._position_of(loader)
    out, states = [], []
    for _ in range(epochs):
        out.append([_qids(b) for b in loader])
        states.append(pos.epoch_state.clone())
    return out, states


@pytest.mark.parametrize("workers", [0, 2])
def test_uninterrupted_loader_yields_the_batches_of_the_parent_construction(tmp_path, workers):
    a = _args(tmp_path, workers)
    ds, loader = T.build_dataloader(a)
    assert isinstance(T._position_of(loader), T._EpochPosition) and len(loader) == STEPS
    # the loader as it was built before the position wrapper existed
    g = torch.Generator()
    g.manual_seed(a.seed + a.rank)
    parent = torch.utils.data.DataLoader(ds, batch_size=a.train_batch_size // a.nranks, shuffle=True, num_workers=workers, collate_fn=ds.collate_fn,
                                         drop_last=True, generator=g, pin_memory=True,
                                         **(dict(prefetch_factor=4, persistent_workers=True) if workers else {}))
    got, _ = _run_epochs(loader, 2)
    want = [[_qids(b) for b in parent] for _ in range(2)]
    assert got == want
    assert got[0] != got[1] and all(len(e) == STEPS and len({q for b in e for q in b}) == 12 for e in got)      # shuffled; every example once
    assert torch.equal(loader.generator.get_state(), g.get_state())                   # and the generator was drawn from equally often


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("epoch", [0, 1])
def test_resumed_loader_yields_the_rest_of_the_epoch_then_the_next_one(tmp_path, workers, epoch, monkeypatch):
    from cldrd_amd.dataset.nway_dataset import NwayDataset
    fetched = []
    real = NwayDataset.__getitem__
    if workers == 0:        # (worker processes would count in their own memory)
        monkeypatch.setattr(NwayDataset, "__getitem__", lambda self, i: (fetched.append(int(i)), real(self, i))[1])
    a = _args(tmp_path, workers)
    _, loader = T.build_dataloader(a)
    full, states = _run_epochs(loader, 3)
    per_batch = [fetched[i:i + 4] for i in range(0, len(fetched), 4)]                  # workers == 0: the example indices of every batch, in order
    assert workers != 0 or len(per_batch) == 3 * STEPS
    for e in range(3):      # a rank that is not rank 0 re-derives the state instead of reading it from the checkpoint: same state
        assert torch.equal(T.replayed_epoch_state(loader, a.seed + a.rank, e), states[e]), e
    del loader
    for s in (0, 1, STEPS - 1, STEPS):                                                   # STEPS: the checkpoint of the epoch's last batch
        _, resumed = T.build_dataloader(a)
        T._position_of(resumed).resume(s, states[epoch])
        del fetched[:]
        got, got_states = _run_epochs(resumed, 2)
        assert got[0] == full[epoch][s:], (s, got[0])
        assert got[1] == full[epoch + 1], s
        assert torch.equal(got_states[0], states[epoch]) and torch.equal(got_states[1], states[epoch + 1])      # what its own checkpoints would hold
        if workers == 0:
            want = [i for b in per_batch[epoch * STEPS + s:(epoch + 2) * STEPS] for i in b]
            assert fetched == want, (s, fetched, want)            # nothing of the batches passed over was fetched
        del resumed


def test_synthetic_loader_skips_whole_batches_by_index():
    a = T.get_args(["--synthetic_steps", "5", "--synthetic_nway", "4", "--query_max_len", "8", "--passage_max_len", "24", "--train_batch_size", "2",
                    "--loss", "kl_div", "--loader_workers", "0"])
    a.rank, a.nranks, a.synthetic_vocab = 0, 1, 512
    made = []
    real = T._SyntheticBatches.__getitem__
    T._SyntheticBatches.__getitem__ = lambda self, i: (made.append(int(i)), real(self, i))[1]
    try:
        loader = T._synthetic_loader(a)
        ds = loader.dataset
        pos = T._position_of(loader)
        assert len(loader) == 5 and pos.generator is None
        pos.resume(3, None)
        first = [b["nway_passages"]["input_ids"] for b in loader]
        second = [b["nway_passages"]["input_ids"] for b in loader]
        assert made == [3, 4, 0, 1, 2, 3, 4] and pos.epoch_state is None
    finally:
        T._SyntheticBatches.__getitem__ = real
    assert len(first) == 2 and len(second) == 5
    assert torch.equal(first[0], ds[3]["nway_passages"]["input_ids"]) and torch.equal(second[0], ds[0]["nway_passages"]["input_ids"])


def test_position_fields_are_compared_one_by_one():
    saved = {"train_batch_size": 8, "nranks": 1, "seed": 4680, "dataset_len": 503000, "steps_per_epoch": 62875, "num_train_epochs": 4}
    assert tuple(saved) == T.POSITION_FIELDS
    T.check_resume_position(dict(saved, epoch=1, step_in_epoch=7), dict(saved))          # equal: no complaint, other keys ignored
    for field in T.POSITION_FIELDS:
        with pytest.raises(ValueError) as err:
            T.check_resume_position(saved, dict(saved, **{field: saved[field] + 1}))
        msg = str(err.value)
        assert field in msg and str(saved[field]) in msg and str(saved[field] + 1) in msg
        assert not any(other in msg for other in T.POSITION_FIELDS if other != field)
        with pytest.raises(ValueError, match=field):
            T.check_resume_position({k: v for k, v in saved.items() if k != field}, saved)


def test_resume_exact_needs_resume(capsys):
    with pytest.raises(SystemExit):
        T.get_args(["--resume_exact"])
    assert "--resume_exact needs --resume" in capsys.readouterr().err
    a = T.get_args(["--resume", "ckpt.pth.tar", "--resume_exact"])
    assert a.resume_exact and not T.get_args(["--resume", "ckpt.pth.tar"]).resume_exact


def test_checkpoint_file_is_moved_into_place(tmp_path, monkeypatch):
    path = os.path.join(str(tmp_path), "checkpoint_5.pth.tar")
    T.save_checkpoint({"global_step": 5}, path)
    assert os.listdir(str(tmp_path)) == ["checkpoint_5.pth.tar"] and torch.load(path)["global_step"] == 5

    def dies(obj, f):
        with open(f, "wb") as fh:
            fh.write(b"half")
        raise KeyboardInterrupt
    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(KeyboardInterrupt):
        T.save_checkpoint({"global_step": 6}, path)
    monkeypatch.undo()
    assert os.listdir(str(tmp_path)) == ["checkpoint_5.pth.tar"] and torch.load(path)["global_step"] == 5      # the old file, whole
