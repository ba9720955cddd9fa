"""PackedRowsDataset: first-fit-decreasing packing of prompt/completion
examples into fixed rows with their document layout."""

import pytest
import torch

from lpp_amd.config import TrainConfig, model_config
from lpp_amd.data import (IGNORE_INDEX, PackedRowsDataset, Seq2SeqToCausalLM,
                          SimpleTokenizer, completion_labels)
from lpp_amd.ops import DocLayout

SEQ = 32


def _corpus(n=40, seed=0, longest=20):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        a = int(torch.randint(1, longest // 2, (1,), generator=g))
        b = int(torch.randint(1, longest // 2, (1,), generator=g))
        out.append({"inputs": " ".join(f"p{i}w{j}" for j in range(a)),
                    "targets": " ".join(f"t{i}w{j}" for j in range(b))})
    return out


def _alone(corpus, seq_len=SEQ):
    """Per example: (ids, labels) as TextCollator's parts give them."""
    tok = SimpleTokenizer(1000)
    enc = Seq2SeqToCausalLM(tok, seq_len)(corpus)
    labels = completion_labels(enc["input_ids"], enc["prompt_lens"], tok.pad_token_id,
                               lengths=enc["lengths"])
    return [(enc["input_ids"][i, :n], labels[i, :n])
            for i, n in enumerate(enc["lengths"].tolist())], tok


def _documents(item):
    """(start, length) of every document of a row, padding singletons included."""
    ds = item["doc_start"].tolist()
    firsts = [i for i, s in enumerate(ds) if s == i] + [len(ds)]
    return [(a, b - a) for a, b in zip(firsts[:-1], firsts[1:])]


def test_every_example_once_rows_full_layout_consistent():
    corpus = _corpus()
    alone, tok = _alone(corpus)
    ds = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ)
    assert ds.num_examples == len(corpus)
    assert sorted(i for row in ds.placement for i in row) == list(range(len(corpus)))
    assert len(ds) == len(ds.placement) < len(corpus)  # it packs
    for r in range(len(ds)):
        item = ds[r]
        assert item["input_ids"].shape == (SEQ,) and item["labels"].shape == (SEQ,)
        assert item["doc_start"].shape == (SEQ,) and item["doc_start"].dtype is torch.int32
        DocLayout(item["doc_start"][None])  # monotone, <= i, starts at 0: validated
        used = sum(alone[i][0].numel() for i in ds.placement[r])
        assert used <= SEQ
        docs = _documents(item)
        at = 0
        for slot, i in enumerate(ds.placement[r]):
            ids, labels = alone[i]
            n = ids.numel()
            assert docs[slot] == (at, n)
            assert torch.equal(item["input_ids"][at:at + n], ids)
            # the example's own completion labels, but no loss on its first token
            assert item["labels"][at] == IGNORE_INDEX
            assert torch.equal(item["labels"][at + 1:at + n], labels[1:])
            at += n
        # the rest is padding: pad ids, no loss, one-token documents
        assert docs[len(ds.placement[r]):] == [(j, 1) for j in range(used, SEQ)]
        assert bool((item["input_ids"][used:] == tok.pad_token_id).all())
        assert bool((item["labels"][used:] == IGNORE_INDEX).all())
    assert ds.real_tokens == sum(a[0].numel() for a in alone)


def test_first_fit_decreasing():
    """Longest first, each into the first row with room."""
    corpus = _corpus(25, seed=3)
    alone, _ = _alone(corpus)
    n = [a[0].numel() for a in alone]
    ds = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ)
    rows, room = [], []
    for i in sorted(range(len(n)), key=lambda i: (-n[i], i)):
        r = next((r for r, free in enumerate(room) if n[i] <= free), None)
        if r is None:
            r = len(room)
            room.append(SEQ)
            rows.append([])
        rows[r].append(i)
        room[r] -= n[i]
    assert ds.placement == rows


def test_two_constructions_identical():
    corpus = _corpus(30, seed=1)
    a = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ)
    b = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ)
    assert a.placement == b.placement and len(a) == len(b)
    for r in range(len(a)):
        for key in ("input_ids", "labels", "doc_start"):
            assert torch.equal(a[r][key], b[r][key])


def test_overlong_example_truncated_not_dropped():
    corpus = _corpus(6, seed=2)
    corpus.insert(2, {"inputs": " ".join(f"a{j}" for j in range(30)),
                      "targets": " ".join(f"b{j}" for j in range(30))})
    ds = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ)
    assert sorted(i for row in ds.placement for i in row) == list(range(7))
    row = next(r for r, members in enumerate(ds.placement) if 2 in members)
    assert ds.placement[row] == [2]  # it fills a row alone
    alone, _ = _alone(corpus)
    assert alone[2][0].numel() == SEQ
    assert torch.equal(ds[row]["input_ids"], alone[2][0])
    assert ds[row]["doc_start"].tolist() == [0] * SEQ


def test_field_and_default_collate():
    corpus = [{"flan": e} for e in _corpus(12, seed=4)]
    ds = PackedRowsDataset(corpus, SimpleTokenizer(1000), SEQ, field="flan")
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert batch["input_ids"].shape == (2, SEQ) and batch["labels"].shape == (2, SEQ)
    assert batch["doc_start"].shape == (2, SEQ) and batch["doc_start"].dtype is torch.int32
    DocLayout(batch["doc_start"])


def test_config_wiring(tmp_path):
    import json

    from lpp_amd.trainer import build_dataset

    cfg = TrainConfig(model=model_config("llama-tiny"), seq_len=SEQ, pack_sequences=True)
    with pytest.raises(ValueError, match="pack_sequences needs data_kind=jsonl"):
        build_dataset(cfg)
    path = tmp_path / "train.jsonl"
    path.write_text("".join(json.dumps(e) + "\n" for e in _corpus(20)))
    cfg = TrainConfig(model=model_config("llama-tiny"), seq_len=SEQ, data_kind="jsonl",
                      train_file=str(path), tokenizer_path="simple", pack_sequences=True)
    ds, collate = build_dataset(cfg)
    assert isinstance(ds, PackedRowsDataset) and len(ds) < 20
    assert collate([ds[0], ds[1]])["doc_start"].shape == (2, SEQ)
    assert TrainConfig.from_dict(cfg.to_dict()).pack_sequences is True
    assert TrainConfig().pack_sequences is False
