"""CPU: the KTH / UCF / BAIR indexes, samplers and host frame pool of dvg_amd/datasets.py against what the reference's own
loaders returned on the tree of tests/clip_tree.py (tests/golden/reference_clips.npz, written by
tests/golden/make_golden_clips.py), and the host-side checks of dvg_clip_gather_u8."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

from dvg_amd import datasets
from tests import clip_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(d, s) for d in ("kth", "ucf", "bair") for s in ("train", "test")]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_clips.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture):
    return clip_tree.build(tmp_path_factory.mktemp("clips"), int(fixture["tree_seed"]))


def host_clip(pool, first, T, channels):
    """The reference's arithmetic on the host pool: imread(f) / 255. in float64 (kth.py:54), channel 0 for KTH (:55)."""
    x = pool[first:first + T].numpy()[..., :channels]
    return (x / 255.).astype(np.float32)


def test_indexes_parse_the_three_tree_formats(tree):
    kth = datasets.open_index("kth", clip_tree.data_root(tree, "kth"), True)
    assert len(kth.videos) == 6 and all(len(v) == 3 and all(len(s) == 2 for s in v) for v in kth.videos)
    assert kth.labels[:6] == [0] * 6 and kth.labels[-1] == 5 and len(kth.sequences) == 36
    assert kth.sequences[0][0].endswith(os.path.join("processed", "boxing", "person01_boxing_d1", "image-000_64x64.png"))
    assert [len(s) for s in kth.sequences[:3]] == list(clip_tree.LENGTHS[:3])
    assert kth.bases[0] == 0 and kth.bases[2] == 14 and kth.n_frames == sum(len(s) for s in kth.sequences)
    kth_test = datasets.open_index("kth", clip_tree.data_root(tree, "kth"), False)
    assert len(kth_test.sequences) == 24 and "person04" in kth_test.sequences[0][0]
    ucf = datasets.open_index("ucf", clip_tree.data_root(tree, "ucf"), True)
    assert len(ucf.videos) == 9 and ucf.labels[-1] == 8 and len(ucf.sequences) == 36
    # ucf.py:13 `train = True`: the test split IS the train split
    ucf_test = datasets.open_index("ucf", clip_tree.data_root(tree, "ucf"), False)
    assert ucf_test.sequences == ucf.sequences and ucf_test.split == "train"
    bair = datasets.open_index("bair", clip_tree.data_root(tree, "bair"), False)
    assert [s[0].split(os.sep)[-3:] for s in bair.sequences] == [
        ["traj_0_to_255", str(i), "0.png"] for i in range(3)] + [["traj_256_to_511", str(i), "0.png"] for i in range(3, 6)]
    assert all(len(s) == clip_tree.BAIR_FRAMES for s in bair.sequences) and set(bair.labels) == {-1}


@pytest.mark.parametrize("dataset,split", CASES)
def test_sampler_and_host_pool_reproduce_the_reference_draws(tree, fixture, dataset, split):
    """40 consecutive draws at T = 8: the labels and the CRC32 of (pool[idx] / 255.).astype(float32) equal what the
    reference's loader returned, and draw 0 equals its clip element for element."""
    T, seed = int(fixture["T"]), int(fixture["seed"])
    index = datasets.open_index(dataset, clip_tree.data_root(tree, dataset), split == "train")
    pool = datasets.build_pool(index, 64, None, threads=4)
    assert pool.dtype == torch.uint8 and tuple(pool.shape) == (index.n_frames, 64, 64, 3)
    sampler = datasets.make_sampler(index, T, seed)
    channels = 1 if dataset == "kth" else 3
    labels, crcs = [], []
    for k in range(len(fixture[f"{dataset}/{split}/crc"])):
        first, label = sampler.draw()
        clip = host_clip(pool, first, T, channels)
        if k == 0:
            assert np.array_equal(clip, fixture[f"{dataset}/{split}/clip0"])
        labels.append(label)
        crcs.append(zlib.crc32(np.ascontiguousarray(clip).tobytes()))
    assert labels == fixture[f"{dataset}/{split}/labels"].tolist()
    assert crcs == fixture[f"{dataset}/{split}/crc"].tolist()


def test_too_short_sequences_are_never_returned(tree):
    for dataset in ("kth", "ucf"):
        index = datasets.open_index(dataset, clip_tree.data_root(tree, dataset), True)
        lengths, bases = index.lengths, index.bases
        assert (lengths < 8).any() and (lengths >= 8).any()
        sampler = datasets.make_sampler(index, 8, 7)
        for _ in range(400):
            first, label = sampler.draw()
            s = int(np.searchsorted(bases, first, side="right")) - 1
            assert lengths[s] >= 8 and first + 8 <= bases[s] + lengths[s] and label == index.labels[s]
        with pytest.raises(SystemExit):
            datasets.make_sampler(index, 17, 7)            # longer than every sequence: would re-draw forever


def test_bair_test_split_walks_in_order_and_wraps_and_train_draws(tree):
    index = datasets.open_index("bair", clip_tree.data_root(tree, "bair"), False)
    sampler = datasets.make_sampler(index, 8, 99)
    firsts = [sampler.draw()[0] for _ in range(14)]
    assert firsts == [clip_tree.BAIR_FRAMES * (k % 6) for k in range(14)]         # every clip starts at frame 0
    train = datasets.open_index("bair", clip_tree.data_root(tree, "bair"), True)
    rng = np.random.RandomState(5)
    s = datasets.make_sampler(train, 8, 5)
    assert [s.draw()[0] for _ in range(20)] == [clip_tree.BAIR_FRAMES * int(rng.randint(6)) for _ in range(20)]
    with pytest.raises(SystemExit, match="fewer than 13"):
        datasets.make_sampler(train, 13, 5)


def test_missing_root_meta_class_and_wrong_frame_size_are_system_exits(tree, tmp_path):
    import shutil
    with pytest.raises(SystemExit, match="no_such_root"):
        datasets.open_index("kth", str(tmp_path / "no_such_root"), True)
    with pytest.raises(SystemExit, match="processed_data"):
        datasets.open_index("bair", str(tmp_path), True)
    broken = tmp_path / "kth"
    shutil.copytree(clip_tree.data_root(tree, "kth"), broken)
    os.remove(broken / "processed" / "running" / "test_meta64x64.json")
    datasets.open_index("kth", str(broken), True)
    with pytest.raises(SystemExit, match="test_meta64x64.json"):
        datasets.open_index("kth", str(broken), False)
    with pytest.raises(SystemExit, match="train_meta128x128.json"):
        datasets.open_index("kth", str(broken), True, image_width=128)
    shutil.rmtree(broken / "processed" / "walking")
    with pytest.raises(SystemExit, match="walking"):
        datasets.open_index("kth", str(broken), True)
    # a frame of another size names its file; so does a frame that is listed but missing
    from PIL import Image
    small = tmp_path / "bair"
    shutil.copytree(clip_tree.data_root(tree, "bair"), small)
    bad = small / "processed_data" / "test" / "traj_0_to_255" / "1" / "3.png"
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(bad)
    index = datasets.open_index("bair", str(small), False)
    with pytest.raises(SystemExit, match=r"1/3\.png.* is 32x32, not 64x64"):
        datasets.build_pool(index, 64, None)
    os.remove(bad)
    Image.fromarray(np.zeros((64, 64), np.uint8)).save(bad)          # mode L in an RGB pool
    with pytest.raises(SystemExit, match="mode L"):
        datasets.build_pool(index, 64, None)
    index.sequences[0][2] = str(small / "gone.png")
    with pytest.raises(SystemExit, match="gone.png"):
        datasets.build_pool(index, 64, None)


def test_mode_l_pngs_make_a_one_channel_pool(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 64, 64), dtype=np.uint8)
    d = tmp_path / "processed_data" / "train" / "a" / "0"
    os.makedirs(d)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(d / f"{i}.png")
    index = datasets.open_index("bair", str(tmp_path), True)
    pool = datasets.build_pool(index, 64, None, threads=100)           # the thread count is capped at 16
    assert tuple(pool.shape) == (5, 64, 64, 1) and np.array_equal(pool.numpy()[..., 0], frames)


def test_float_division_by_255_equals_the_reference_path_for_every_byte():
    """The kernel's arithmetic: float32(v) / float32(255), correctly rounded, is bit-equal to the reference's
    float32(float64(v) / 255.) for all 256 byte values; the multiply by float32(1/255) is not."""
    v = np.arange(256)
    ref = (v.astype(np.float64) / 255.).astype(np.float32)
    div = v.astype(np.float32) / np.float32(255)
    mul = v.astype(np.float32) * (np.float32(1) / np.float32(255))
    assert div.dtype == np.float32 and np.array_equal(div.view(np.uint32), ref.view(np.uint32))
    assert int((mul.view(np.uint32) == ref.view(np.uint32)).sum()) == 130


def test_clip_gather_host_checks_reject_bad_calls_without_gpu():
    """dvg_clip_gather_u8 checks its arguments on the host before any launch (fake pointers, never dereferenced)."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = dict(n=100, T=8, B=4, C=1, H=64, W=64, pc=1)

    def call(pool=one, first=one, out=one, **kw):
        a = dict(ok, **kw)
        return lib.dvg_clip_gather_u8(pool, first, out, a["n"], a["T"], a["B"], a["C"], a["H"], a["W"], a["pc"], None)
    SHAPE, NULL, ALIGN = 1, 2, 4
    assert call(pool=None) == NULL and call(first=None) == NULL and call(out=None) == NULL
    for zero in ("T", "B", "C", "H", "W"):
        assert call(**{zero: 0}) == SHAPE, zero
    for c, pc in ((3, 1), (2, 2), (2, 3), (1, 4), (4, 4), (1, 0)):
        assert call(C=c, pc=pc) == SHAPE and b"pool of" in lib.dvg_last_error(), (c, pc)
    assert call(n=7) == SHAPE                                            # fewer frames than one clip
    assert call(W=24) == SHAPE and b"multiple of 16" in lib.dvg_last_error()       # the choice: no scalar tail path
    assert call(W=40, C=3, pc=3) == SHAPE                                # 120 bytes per row
    assert call(n=5000, T=2048, B=256, C=3, pc=3) == SHAPE and b"32-bit offsets" in lib.dvg_last_error()
    assert call(pool=ctypes.c_void_p(24)) == ALIGN and call(out=ctypes.c_void_p(8)) == ALIGN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        from dvg_amd import ops
        ops.clip_gather(torch.zeros(10, 64, 64, 1, dtype=torch.uint8), np.zeros(2, np.int64), 4, 1)
