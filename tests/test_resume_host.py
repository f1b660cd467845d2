"""CPU: the host half of `train.py --resume` - the data position of every sampler and of the prefetcher in front of them, the
argument surface, and the one-line refusals of a state file that is missing, truncated or from another configuration."""
import os
import types

import numpy as np
import pytest
import torch

from dvg_amd import data, datasets, mnist, train_state
from dvg_amd.train_graphs import BatchPrefetcher
from tests import clip_tree, mnist_tree

K, M, B, T = 3, 4, 3, 8


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    return clip_tree.build(tmp_path_factory.mktemp("resume_clips"), 0)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _samplers(clips):
    """name -> (factory of a fresh sampler, draw of one batch's host half)."""
    def clip(dataset, train):
        index = datasets.open_index(dataset, clip_tree.data_root(clips, dataset), train)
        return (lambda: datasets.make_sampler(index, T, 11)), (lambda s: [s.draw() for _ in range(B)])
    return {
        "meta-kth": clip("kth", True),            # MetaSampler: numpy stream + Python stream, re-draws of short sequences
        "meta-ucf": clip("ucf", True),
        "bair-random": clip("bair", True),        # BairSampler, random walk
        "bair-ordered": clip("bair", False),      # BairSampler, ordered walk that wraps (6 directories, 21 draws)
        "mnist": ((lambda: mnist.MovingMnistSampler(mnist_tree.N_TRAIN, T, 2, 64, 11)), (lambda s: s.draw(B))),
        "synthetic": ((lambda: data.SyntheticMovingMNIST(seq_len=T, num_digits=2, image_size=64, seed=11, n_sprites=4)),
                      (lambda s: s.trajectories(B))),
    }


@pytest.mark.parametrize("name", ["meta-kth", "meta-ucf", "bair-random", "bair-ordered", "mnist", "synthetic"])
def test_sampler_position_restores_the_stream(clips, name):
    """Draw K batches, take the position, restore it into a FRESH sampler: the next M draws are the uninterrupted sampler's,
    integer for integer - and they are not what a fresh sampler draws without the restore (the check can fail)."""
    make, draw = _samplers(clips)[name]
    a = make()
    assert isinstance(a, {"meta": datasets.MetaSampler, "bair": datasets.BairSampler, "mnist": mnist.MovingMnistSampler,
                          "synthetic": data.SyntheticMovingMNIST}[name.split("-")[0]])
    if name.startswith("bair"):
        assert a.ordered == (name == "bair-ordered")
    for _ in range(K):
        draw(a)
    pos = a.position()
    want = [draw(a) for _ in range(M)]
    assert not _same(a.position(), pos) or name == "bair-ordered"       # the position taken is a copy, not a live view
    b = make()
    b.restore(torch.load(_roundtrip(pos), weights_only=False))          # as it comes back from a state file
    got = [draw(b) for _ in range(M)]
    assert _same(got, want)
    fresh = make()
    assert not _same([draw(fresh) for _ in range(M)], want)


def _roundtrip(obj):
    import io
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return f


def test_a_position_of_another_sampler_is_refused(clips):
    make, _ = _samplers(clips)["mnist"]
    other, _ = _samplers(clips)["bair-random"]
    with pytest.raises(SystemExit, match="saved for BairSampler, this run draws from MovingMnistSampler"):
        make().restore(other().position())
    with pytest.raises(SystemExit, match="saved for MovingMnistSampler, this run draws from MetaSampler"):
        _samplers(clips)["meta-kth"][0]().restore(make().position())


def _opt(dataset="smmnist", synthetic=False):
    return types.SimpleNamespace(dataset=dataset, data_root="path/to/data/", image_width=64, channels=1, local_batch=B, rank=1,
                                 num_digits=2, synthetic_data=synthetic)


def _stream(monkeypatch, dataset="smmnist"):
    """make_batch_generator's synthetic streams with the device half replaced by the identity: load() returns the host half."""
    monkeypatch.setattr(data.SyntheticMovingMNIST, "compose_device", lambda self, ids, pos, device: (ids, pos))
    monkeypatch.setattr(data, "normalize_data", lambda opt, dtype, seq: (seq.numpy(),))
    return data.make_batch_generator(_opt(dataset, dataset != "smmnist"), T, 21, device="cpu")


@pytest.mark.parametrize("dataset", ["smmnist", "kth"])
def test_batch_stream_position_is_that_of_the_last_batch_handed_out(monkeypatch, dataset):
    """smmnist: SyntheticMovingMNIST's generator; kth + --synthetic_data: the `seed + k` stream of textured clips."""
    a = _stream(monkeypatch, dataset)
    assert isinstance(a, data.BatchStream)
    start = a.position()
    first = [next(a)() for _ in range(K)]
    pos = a.position()
    want = [next(a)() for _ in range(M)]
    b = _stream(monkeypatch, dataset)
    b.restore(pos)
    assert _same([next(b)() for _ in range(M)], want)
    b.restore(start)
    assert _same([next(b)() for _ in range(K)], first)


@pytest.mark.parametrize("dataset", ["smmnist", "kth"])
def test_prefetcher_position_counts_consumed_batches_not_drawn_ones(monkeypatch, dataset):
    """A BatchPrefetcher of depth 2 draws up to three batches ahead.  The position after CONSUMING K batches restores to batch
    K + 1 - not to K + 3, where the sampler stands once the thread has filled its queue."""
    plain = _stream(monkeypatch, dataset)
    all_ = [next(plain)() for _ in range(K + M + 4)]
    gen = _stream(monkeypatch, dataset)
    pf = BatchPrefetcher(gen, depth=2)
    start = pf.position()
    for k in range(K):
        assert _same(next(pf)(), all_[k])
    while pf.q.qsize() < 2:             # let the thread run ahead as far as it can: two queued (+ one drawn, waiting in put)
        pf.thread.join(0.001)
    pos = pf.position()
    assert not _same(pos, gen.sampler.position())            # the sampler itself is ahead of the consumer
    fresh = BatchPrefetcher(_stream(monkeypatch, dataset), depth=2)
    fresh.restore(torch.load(_roundtrip(pos), weights_only=False))
    got = [next(fresh)() for _ in range(M)]
    assert _same(got, all_[K:K + M]) and not _same(got, all_[K + 2:K + 2 + M]) and not _same(got, all_[K + 3:K + 3 + M])
    # the same prefetcher can be taken back as well (its thread is stopped and restarted), here to the very beginning
    pf.restore(start)
    assert _same([next(pf)() for _ in range(K + 1)], all_[:K + 1])
    assert _same(pf.position(), next(x for i, x in enumerate(_positions(monkeypatch, dataset)) if i == K))


def _positions(monkeypatch, dataset):
    s = _stream(monkeypatch, dataset)
    while True:
        yield next(s).position


def test_prefetcher_in_front_of_a_plain_iterator_has_no_position():
    pf = BatchPrefetcher(iter(range(5)), depth=2)
    assert pf.position() is None and list(pf) == list(range(5)) and pf.position() is None


# ---- the argument surface and the refusals --------------------------------------------------------------------------
def test_resume_parses_and_model_dir_stays_unused():
    import train
    p = train.build_parser()
    assert p.parse_args([]).resume == "" and p.parse_args(["--resume", "out/train_state.pth"]).resume == "out/train_state.pth"
    assert p.parse_args(["--model_dir", "x"]).model_dir == "x"
    text = " ".join(p.format_help().split())          # (argparse wraps the help text)
    assert "accepted and unused, as in the reference" in text and "--resume PATH" in text


def _state(**over):
    opt = types.SimpleNamespace(model="dcgan", image_width=64, channels=1, g_dim=90, rnn_size=256, predictor_rnn_layers=2,
                                batch_size=4, n_past=2, n_future=2, n_eval=4, dataset="smmnist", num_digits=2, last_frame_skip=False,
                                ft=True, world=1)
    fp = train_state.option_fingerprint(opt)
    fp["layout"] = [["gp", 0, 0, 8], ["gp", 1, 8, 12]]
    sd = {"format": train_state.FORMAT, "fingerprint": fp, "epoch": 2, "global_step": 4, "arena": {}, "optimizers": {},
          "scheduler": {}, train_state.RANK_KEY: {"rank": 0, "buffers": {}, "rng": {}, "plot_writer": None, "data": {}}}
    sd.update(over)
    return sd, opt


ARGS = ["--model", "dcgan", "--batch_size", "4", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--dataset", "smmnist",
        "--no_save"]


def test_resolve_takes_a_file_or_its_directory(tmp_path):
    f = str(tmp_path / "train_state.pth")
    assert train_state.resolve(str(tmp_path)) == f and train_state.resolve(f) == f
    assert train_state.rank_path(f, 3) == str(tmp_path / "train_state.rank3.pth")


def test_atomic_save_leaves_the_previous_file_when_the_write_dies(tmp_path, monkeypatch):
    f = str(tmp_path / "train_state.pth")
    train_state.atomic_save({"v": 1}, f)

    def dies(obj, path):
        with open(path, "wb") as fh:
            fh.write(b"half a fi")
        raise KeyboardInterrupt
    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(KeyboardInterrupt):
        train_state.atomic_save({"v": 2}, f)
    monkeypatch.undo()
    assert torch.load(f, weights_only=False) == {"v": 1} and os.listdir(str(tmp_path)) == ["train_state.pth"]


@pytest.mark.parametrize("field,flag,value", [("n_past", "--n_past", "3"), ("batch_size", "--batch_size", "8"),
                                              ("model", "--model", "vgg"), ("g_dim", "--g_dim", "64"),
                                              ("ft", "--no_ft", None)])
def test_main_refuses_a_state_of_another_configuration_naming_the_field(tmp_path, field, flag, value):
    """Checked before anything is built (no GPU needed to be told): SystemExit, one line, the field by name."""
    import train
    sd, opt = _state()
    f = str(tmp_path / "train_state.pth")
    torch.save(sd, f)
    with pytest.raises(SystemExit) as e:
        train.main(ARGS + [flag] + ([value] if value is not None else []) + ["--resume", str(tmp_path)])
    msg = str(e.value)
    now = {"ft": False, "model": "vgg"}.get(field, int(value) if value and value.isdigit() else value)
    assert msg == f"train.py --resume: {f}: {field} is {getattr(opt, field)!r} in the file and {now!r} in this run"
    assert "\n" not in msg


def test_layout_and_world_mismatches_name_their_field(tmp_path):
    sd, opt = _state()
    f = str(tmp_path / "train_state.pth")
    with pytest.raises(SystemExit, match="train_state.pth: layout is .* in the file and .* in this run"):
        train_state.check_fingerprint(sd["fingerprint"], dict(sd["fingerprint"], layout=[["gp", 0, 0, 8], ["gp", 1, 8, 16]]), f)
    train_state.check_fingerprint(sd["fingerprint"], {"layout": [("gp", 0, 0, 8), ("gp", 1, 8, 12)]}, f)   # tuples or lists
    torch.save(sd, f)
    with pytest.raises(SystemExit, match="train_state.pth: world is 1 in the file and 2 in this run"):
        train_state.read(f, rank=0, world=2)
    assert train_state.read(f)["epoch"] == 2


def test_main_refuses_a_missing_a_truncated_and_a_foreign_file(tmp_path):
    import train
    sd, _ = _state()
    sd["arena"] = {"p": torch.arange(5000.0)}
    f = str(tmp_path / "train_state.pth")
    with pytest.raises(SystemExit) as e:
        train.main(ARGS + ["--resume", f])
    assert str(e.value) == f"train.py --resume: {f}: no such file"
    torch.save(sd, f)
    whole = open(f, "rb").read()
    for cut in (len(whole) // 2, 10, 0):
        with open(f, "wb") as fh:
            fh.write(whole[:cut])
        with pytest.raises(SystemExit) as e:
            train.main(ARGS + ["--resume", f])
        assert str(e.value).startswith(f"train.py --resume: {f}: cannot be read, truncated or not a training state (")
        assert "\n" not in str(e.value)
    torch.save({"encoder": 1}, f)                      # a model.pth is not a training state
    with pytest.raises(SystemExit, match="train_state.pth: format is None in the file and 1 in this run"):
        train.main(ARGS + ["--resume", f])
    del sd["scheduler"]
    torch.save(sd, f)
    with pytest.raises(SystemExit, match="train_state.pth: no field 'scheduler'"):
        train.main(ARGS + ["--resume", f])


def test_rank_files_of_another_epoch_are_refused(tmp_path):
    sd, _ = _state()
    sd["fingerprint"]["world"] = 2
    d = str(tmp_path)
    for r in (0, 1):
        train_state.write(dict(sd), d, r, 2)
    assert sorted(os.listdir(d)) == ["train_state.pth", "train_state.rank0.pth", "train_state.rank1.pth"]
    shared = torch.load(os.path.join(d, "train_state.pth"), weights_only=False)
    assert train_state.RANK_KEY not in shared                      # what differs per rank is in the rank files only
    assert train_state.read(os.path.join(d, "train_state.pth"), 1, 2)[train_state.RANK_KEY]["rank"] == 0   # (fixture's value)
    stale = dict(sd, epoch=1)
    train_state.write(stale, d, 1, 2)
    with pytest.raises(SystemExit, match=r"train_state.rank1.pth: epoch is 1 in the file and 2 in train_state.pth"):
        train_state.read(os.path.join(d, "train_state.pth"), 1, 2)
    os.remove(os.path.join(d, "train_state.rank1.pth"))
    with pytest.raises(SystemExit, match=r"train_state.rank1.pth: no such file"):
        train_state.read(os.path.join(d, "train_state.pth"), 1, 2)
