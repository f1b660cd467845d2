"""CPU: the host half of `train.py --augment` - the spec parser, the pinned draw order of datasets.ClipAugmenter, its position
inside the data position of a BatchStream, the untouched clip selection, and the host checks of dvg_clip_gather_aug_u8."""
import ctypes
import io
import types

import numpy as np
import pytest
import torch

from dvg_amd import data, datasets, ops, train_state
from dvg_amd.train_graphs import BatchPrefetcher
from tests import clip_tree

B, T = 3, 8
FULL = "hflip,reverse,shift=3,jitter=0.2"


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    return clip_tree.build(tmp_path_factory.mktemp("augment_clips"), 0)


def test_parse_augment_canonicalises_and_refuses():
    cfg = datasets.parse_augment(" jitter=0.25, shift=16,reverse ,hflip")
    assert cfg == {"hflip": True, "reverse": True, "shift": 16, "jitter": 0.25}
    assert datasets.augment_spec(cfg) == "hflip,reverse,shift=16,jitter=0.25"
    assert datasets.augment_spec(datasets.parse_augment("shift=1")) == "shift=1"
    assert datasets.augment_spec(datasets.parse_augment("jitter=0.5,hflip")) == "hflip,jitter=0.5"
    assert datasets.parse_augment("") == {"hflip": False, "reverse": False, "shift": 0, "jitter": 0.0}
    assert datasets.augment_spec(datasets.parse_augment("")) == ""
    for bad, named in (("rotate", "rotate"), ("hflip,hflip", "hflip"), ("shift=2,shift=3", "shift"), ("shift=0", "shift=0"),
                       ("shift=17", "shift=17"), ("jitter=0.6", "jitter=0.6"), ("jitter=0", "jitter=0"), ("shift", "shift"),
                       ("hflip=1", "hflip=1"), ("shift=x", "shift=x"), ("jitter=nan", "jitter=nan"), ("hflip,", "''")):
        with pytest.raises(SystemExit) as e:
            datasets.parse_augment(bad)
        assert named in str(e.value) and "\n" not in str(e.value), bad


def test_draw_order_is_pinned():
    """hflip,shift=2,jitter=0.1 with seed 5: per clip randint(2), randint(-2, 3) twice (dy, then dx), uniform(-G, G) twice."""
    geom, photo = datasets.ClipAugmenter("hflip,shift=2,jitter=0.1", 5).draw(3)
    rng = np.random.RandomState(5)
    want_g, want_p = np.zeros((3, 4), np.int32), np.zeros((3, 2), np.float32)
    for i in range(3):
        want_g[i, 0] = rng.randint(2)
        want_g[i, 2] = rng.randint(-2, 3)
        want_g[i, 3] = rng.randint(-2, 3)
        c = 1 + rng.uniform(-0.1, 0.1)
        b = rng.uniform(-0.1, 0.1) / 2
        want_p[i] = np.float32(c), np.float32(0.5 - 0.5 * c + b)
    assert geom.dtype == np.int32 and photo.dtype == np.float32
    assert np.array_equal(geom, want_g) and np.array_equal(photo.view(np.uint32), want_p.view(np.uint32))
    assert (geom[:, 1] == 0).all() and len(set(map(tuple, geom))) > 1
    # one transform less consumes fewer draws: the same seed, another stream from the second clip on
    g2, p2 = datasets.ClipAugmenter("hflip,jitter=0.1", 5).draw(3)
    rng = np.random.RandomState(5)
    for i in range(3):
        assert g2[i, 0] == rng.randint(2) and (g2[i, 1:] == 0).all()
        c = 1 + rng.uniform(-0.1, 0.1)
        b = rng.uniform(-0.1, 0.1) / 2
        assert p2[i, 0] == np.float32(c) and p2[i, 1] == np.float32(0.5 - 0.5 * c + b)
    # disabled transforms: identity parameters, and no draw at all
    a = datasets.ClipAugmenter("reverse", 5)
    g3, p3 = a.draw(4)
    rng = np.random.RandomState(5)
    assert g3[:, 1].tolist() == [rng.randint(2) for _ in range(4)] and (g3[:, [0, 2, 3]] == 0).all()
    assert np.array_equal(p3, np.tile(np.float32([1.0, 0.0]), (4, 1)))
    # the ranges: shift covers [-N, N], the jitter keeps gain within 1 +- G
    g4, p4 = datasets.ClipAugmenter("shift=16,jitter=0.5", 1).draw(400)
    assert g4[:, 2:].min() == -16 and g4[:, 2:].max() == 16
    assert 0.5 <= p4[:, 0].min() < 0.6 and 1.4 < p4[:, 0].max() <= 1.5


def _roundtrip(obj):
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f, weights_only=False)


def test_augmenter_position_survives_a_file_and_refuses_another_spec():
    a = datasets.ClipAugmenter(FULL, 9)
    a.draw(5)
    pos = a.position()
    assert pos["spec"] == FULL
    want = [a.draw(4) for _ in range(3)]
    b = datasets.ClipAugmenter(FULL, 1234)
    b.restore(_roundtrip(pos))
    for (g, p), (wg, wp) in zip([b.draw(4) for _ in range(3)], want):
        assert np.array_equal(g, wg) and np.array_equal(p.view(np.uint32), wp.view(np.uint32))
    fresh = datasets.ClipAugmenter(FULL, 9).draw(4)
    assert not np.array_equal(fresh[1], want[0][1])
    with pytest.raises(SystemExit) as e:
        datasets.ClipAugmenter("hflip", 9).restore(pos)
    assert FULL in str(e.value) and "'hflip'" in str(e.value) and "\n" not in str(e.value)


class _Host:
    """What the patched gathers return: the host half as handed to the op."""

    def __init__(self, *host):
        self.host = host

    def unbind(self, dim):
        return self.host


def _opt(clips, dataset="kth", augment=""):
    return types.SimpleNamespace(dataset=dataset, data_root=clip_tree.data_root(clips, dataset), image_width=64,
                                 channels=1 if dataset == "kth" else 3, local_batch=B, rank=0, data_threads=4,
                                 synthetic_data=False, augment=augment)


def _stream(monkeypatch, clips, augment="", dataset="kth", train=True, seed=21):
    """make_batch_generator over the host pool with the device half replaced by the identity: load() returns the host half
    ((first,) without augmentation, (first, geom, photo) with)."""
    monkeypatch.setattr(ops, "clip_gather", lambda pool, first, T_, C: _Host(first))
    monkeypatch.setattr(ops, "clip_gather_aug", lambda pool, first, geom, photo, T_, C: _Host(first, geom, photo))
    return data.make_batch_generator(_opt(clips, dataset, augment), T, seed, device="cpu", train=train)


@pytest.mark.parametrize("dataset", ["kth", "bair"])
def test_augmentation_leaves_the_clip_selection_alone(monkeypatch, clips, dataset):
    plain = _stream(monkeypatch, clips, "", dataset)
    aug = _stream(monkeypatch, clips, FULL, dataset)
    assert plain.augmenter is None and aug.augmenter is not None and aug.augmenter.spec == FULL
    twin = datasets.ClipAugmenter(FULL, 21 ^ datasets.AUGMENT_SEED_XOR)
    firsts = []
    for _ in range(6):
        (f0,), (f1, geom, photo) = next(plain)(), next(aug)()
        assert f0.dtype == np.int64 and np.array_equal(f0, f1)
        wg, wp = twin.draw(B)
        assert np.array_equal(geom, wg) and np.array_equal(photo.view(np.uint32), wp.view(np.uint32))
        firsts.append(f0)
    assert len({tuple(f) for f in firsts}) > 1


def test_the_test_split_ignores_the_option(monkeypatch, clips):
    gen = _stream(monkeypatch, clips, FULL, train=False)
    plain = _stream(monkeypatch, clips, "", train=False)
    assert gen.augmenter is None and "augment" not in gen.position()
    for _ in range(3):
        got, want = next(gen)(), next(plain)()
        assert len(got) == 1 and np.array_equal(got[0], want[0])


def test_stream_position_carries_the_augmenter_and_restores_both(monkeypatch, clips):
    a = _stream(monkeypatch, clips, FULL)
    assert a.position()["augment"]["spec"] == FULL and a.position()["sampler"] == "MetaSampler"
    for _ in range(3):
        next(a)()
    pos = _roundtrip(a.position())
    want = [next(a)() for _ in range(4)]
    b = _stream(monkeypatch, clips, FULL)
    b.restore(pos)
    for got, w in zip([next(b)() for _ in range(4)], want):
        assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(got, w)) and len(got) == 3
    # behind a prefetcher the position is still that of the last batch CONSUMED, augmenter included
    plain = _stream(monkeypatch, clips, FULL)
    all_ = [next(plain)() for _ in range(8)]
    pf = BatchPrefetcher(_stream(monkeypatch, clips, FULL), depth=2)
    for k in range(3):
        assert np.array_equal(next(pf)()[2], all_[k][2])
    while pf.q.qsize() < 2:
        pf.thread.join(0.001)
    fresh = BatchPrefetcher(_stream(monkeypatch, clips, FULL), depth=2)
    fresh.restore(_roundtrip(pf.position()))
    for k in range(3, 6):
        got = next(fresh)()
        assert all(np.array_equal(u, v) for u, v in zip(got, all_[k]))


def test_stream_restore_refusals(monkeypatch, clips):
    aug, plain = _stream(monkeypatch, clips, FULL), _stream(monkeypatch, clips, "")
    with pytest.raises(SystemExit) as e:
        aug.restore(plain.position())
    assert str(e.value) == f"data position: saved without --augment, this run has --augment {FULL!r}"
    with pytest.raises(SystemExit) as e:
        plain.restore(aug.position())
    assert str(e.value) == f"data position: saved with --augment {FULL!r}, this run has no --augment"
    with pytest.raises(SystemExit, match="saved with --augment .* this run has --augment 'hflip'"):
        _stream(monkeypatch, clips, "hflip").restore(aug.position())


def test_the_flag_is_not_part_of_the_resume_fingerprint_and_is_refused_where_nothing_is_augmented():
    import train
    p = train.build_parser()
    args = ["--dataset", "kth", "--data_root", "x"]
    a, b = p.parse_args(args), p.parse_args(args + ["--augment", "jitter=0.1,hflip"])
    assert a.augment == "" and datasets.check_augment(a) == "" and datasets.check_augment(b) == "hflip,jitter=0.1"
    for o in (a, b):
        o.ft, o.world = True, 1
    assert train_state.option_fingerprint(a) == train_state.option_fingerprint(b)
    for extra, named in ((["--dataset", "smmnist"], "--dataset smmnist"), (["--dataset", "kth", "--synthetic_data"], "--synthetic_data")):
        with pytest.raises(SystemExit) as e:
            train.main(extra + ["--augment", "hflip"])
        assert str(e.value).startswith("train.py --augment:") and named in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit, match="unknown word 'rotate'"):
        train.main(["--dataset", "kth", "--augment", "rotate"])


def test_clip_gather_aug_host_checks_reject_bad_calls_without_gpu():
    """dvg_clip_gather_aug_u8 checks its arguments on the host before any launch (fake pointers, never dereferenced)."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = dict(n=100, T=8, B=4, C=1, H=64, W=64, pc=1)

    def call(pool=one, first=one, geom=one, photo=one, out=one, **kw):
        a = dict(ok, **kw)
        return lib.dvg_clip_gather_aug_u8(pool, first, geom, photo, out, a["n"], a["T"], a["B"], a["C"], a["H"], a["W"], a["pc"],
                                          None)
    SHAPE, NULL, ALIGN = 1, 2, 4
    assert call(pool=None) == NULL and call(first=None) == NULL and call(out=None) == NULL
    assert call(geom=None) == NULL and b"geom" in lib.dvg_last_error()
    assert call(photo=None) == NULL
    assert call(photo=ctypes.c_void_p(18)) == ALIGN and b"4-byte" in lib.dvg_last_error()
    assert call(geom=ctypes.c_void_p(17)) == ALIGN
    for zero in ("T", "B", "C", "H", "W"):
        assert call(**{zero: 0}) == SHAPE, zero
    assert call(C=3, pc=1) == SHAPE and b"pool of" in lib.dvg_last_error()           # C = 3 from a 1-channel pool
    assert call(C=2, pc=3) == SHAPE
    assert call(n=7) == SHAPE                                                        # fewer frames than one clip
    assert call(W=24) == SHAPE and b"multiple of 16" in lib.dvg_last_error()
    assert call(W=40, C=3, pc=3) == SHAPE                                            # 120 bytes per row
    assert call(W=2048, H=4) == SHAPE and b"exceeds" in lib.dvg_last_error()         # a row must fit a tile
    assert call(n=5000, T=2048, B=256, C=3, pc=3) == SHAPE and b"32-bit offsets" in lib.dvg_last_error()
    assert call(pool=ctypes.c_void_p(24)) == ALIGN and call(out=ctypes.c_void_p(8)) == ALIGN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_gather_aug(torch.zeros(10, 64, 64, 1, dtype=torch.uint8), np.zeros(2, np.int64), np.zeros((2, 4), np.int32),
                            np.ones((2, 2), np.float32), 4, 1)
