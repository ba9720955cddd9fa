"""Sequence packing through the pipeline on gloo: the document layout rides
the forward channel behind the hidden state, and PP=2 reproduces the
single-process trajectory on packed rows."""

import torch
from torch.utils.data import DataLoader

from lpp_amd.data import PackedRowsDataset, RepeatingLoader, SimpleTokenizer
from tests.dist_utils import run_dist
from tests.engine_utils import build_engine, make_config, sequential_loader


class _NumberTokenizer(SimpleTokenizer):
    """Words are decimal numbers and map to themselves: the same ids in every
    process (SimpleTokenizer hashes words, and str hashes differ per process)."""

    def _tok(self, word):
        return self._special[word] if word in self._special else 4 + int(word) % 250


def _corpus(n=48):
    g = torch.Generator().manual_seed(21)
    out = []
    for _ in range(n):
        a, b = (int(x) for x in torch.randint(1, 9, (2,), generator=g))
        words = [str(int(x)) for x in torch.randint(0, 250, (a + b,), generator=g)]
        out.append({"inputs": " ".join(words[:a]), "targets": " ".join(words[a:])})
    return out


def _packed_loader(cfg):
    ds = PackedRowsDataset(_corpus(), _NumberTokenizer(cfg.model.vocab_size), cfg.seq_len)
    assert len(ds) >= cfg.micro_batch_size and ds.num_examples > 2 * len(ds)
    loader = DataLoader(ds, batch_size=cfg.micro_batch_size, shuffle=False, drop_last=True)
    return iter(RepeatingLoader(loader))


def _run_packed(rank, world_size, num_stages, steps, gas, pack=True):
    cfg = make_config(num_stages=num_stages, gas=gas)
    cfg.pack_sequences = pack
    engine = build_engine(cfg, rank, world_size)
    needs_data = engine.is_first_stage or engine.is_last_stage
    if pack:
        it = _packed_loader(cfg) if needs_data else None
    else:
        it = sequential_loader(cfg) if needs_data else None
    losses = [float(engine.train_batch(it)) for _ in range(steps)]
    eval_loss = float(engine.eval_batch(it, micro_batches=2))
    return losses, eval_loss, engine.p2p.fwd_messages_sent


def test_pp2_packed_matches_single_process():
    """As exactly as the unpacked PP2 test asserts it (tests/test_pipeline_gloo.py)."""
    steps, gas = 3, 4
    base, base_eval, _ = _run_packed(0, 1, 1, steps, gas)
    got = run_dist(2, _run_packed, 2, steps, gas)
    for r in range(2):
        losses, eval_loss, _ = got[r]
        for a, b in zip(base, losses):
            assert abs(a - b) < 1e-4, (base, losses)
        assert abs(base_eval - eval_loss) < 1e-4
    # hidden state + doc_start per microbatch from the first stage, none from the last
    assert got[0][2] == 2 * (steps * gas + 2)
    assert got[1][2] == 0


def test_packing_changes_the_trajectory():
    """The layout is in use: the same rows trained as one document each give
    other losses."""
    cfg = make_config(num_stages=1, gas=2)
    cfg.pack_sequences = True
    engine = build_engine(cfg, 0, 1)
    packed = float(engine.train_batch(_packed_loader(cfg)))

    def one_document(it):
        for batch in it:
            batch = dict(batch)
            batch["doc_start"] = torch.zeros_like(batch["doc_start"])
            yield batch

    engine = build_engine(cfg, 0, 1)
    mixed = float(engine.train_batch(one_document(_packed_loader(cfg))))
    assert abs(packed - mixed) > 1e-3, (packed, mixed)


def test_packing_off_sends_one_message_per_microbatch():
    steps, gas = 2, 4
    got = run_dist(2, _run_packed, 2, steps, gas, False)
    assert got[0][2] == steps * gas + 2  # + the two eval microbatches
    assert got[1][2] == 0
