"""CPU: Moving-MNIST from real digits, the host half (dvg_amd/mnist.py) - the IDX reader, the restated Pillow resize, the
reference's draw order and compositing - against what the reference's data/moving_mnist.py returned on the tree of
tests/mnist_tree.py (tests/golden/reference_mnist.npz, written by tests/golden/make_golden_mnist.py); and the fallback of
make_batch_generator without MNIST files."""
import os
import struct
import types
import zlib

import numpy as np
import pytest

from dvg_amd import data, mnist
from tests import mnist_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_mnist.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture):
    return mnist_tree.build(tmp_path_factory.mktemp("mnist"), int(fixture["tree_seed"]))


@pytest.mark.parametrize("sub", [("MNIST", "raw"), ("raw",), ()])
@pytest.mark.parametrize("gz", [False, True])
def test_reader_accepts_the_three_layouts_raw_and_gzipped(tmp_path, sub, gz):
    imgs = {t: mnist_tree.images(3, t) for t in (True, False)}
    for t in (True, False):
        assert mnist.find_tree(tmp_path, t) is None                           # both splits' files are asked for
        mnist_tree.write(os.path.join(str(tmp_path), *sub), t, imgs[t], gz)
    for t in (True, False):
        path = mnist.find_tree(tmp_path, t)
        assert path == os.path.join(str(tmp_path), *sub, mnist_tree.NAMES[t] + (".gz" if gz else ""))
        assert path in mnist.candidates(str(tmp_path), t)
        got = mnist.read_idx_images(path)
        assert got.dtype == np.uint8 and np.array_equal(got, imgs[t])


def test_reader_rejects_a_wrong_magic_a_truncated_file_and_a_non_square_header(tmp_path):
    imgs = mnist_tree.images(0, False)
    good = mnist_tree.idx_bytes(imgs)
    cases = {"magic": struct.pack(">I", 0x00000801) + good[4:],               # the label files' magic
             "truncated": good[:-5],
             "longer": good + b"\0",
             "header": good[:9],
             "non-square": struct.pack(">IIII", mnist_tree.MAGIC, len(imgs) * 2, 14, 28) + good[16:]}
    for name, blob in cases.items():
        path = os.path.join(str(tmp_path), name + "-idx3-ubyte")
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(ValueError, match=name + "-idx3-ubyte"):
            mnist.read_idx_images(path)
    bad_gz = os.path.join(str(tmp_path), "broken-idx3-ubyte.gz")
    with open(bad_gz, "wb") as f:
        f.write(good)                                                         # not gzipped at all
    with pytest.raises(ValueError, match="broken-idx3-ubyte.gz"):
        mnist.read_idx_images(bad_gz)
    with pytest.raises(ValueError, match="missing-file"):
        mnist.read_idx_images(os.path.join(str(tmp_path), "missing-file"))


def test_numpy_resize_equals_the_fixture_sprites_and_pillow(fixture):
    seed = int(fixture["tree_seed"])
    for train, split in ((True, "train"), (False, "test")):
        assert np.array_equal(mnist.resize_u8(mnist_tree.images(seed, train)), fixture[f"{split}/sprites"])
    same = mnist_tree.images(seed, False)
    assert np.array_equal(mnist.resize_u8(same, 28), same)                    # in_size == out_size: the identity
    with pytest.raises(ValueError, match="up-scaling"):
        mnist.resize_tables(32, 28)
    xmin, coef = mnist.resize_tables(28, 32)
    assert xmin.min() >= 0 and (xmin + (coef != 0).sum(1)).max() <= 28 and (coef != 0).sum(1).max() <= 2
    assert np.abs(coef.sum(1) - (1 << 22)).max() <= 1
    try:
        from PIL import Image
    except ImportError:                                                       # the fixture's sprites ARE Pillow's output
        return
    rng = np.random.default_rng(11)
    for s, o in ((28, 32), (28, 64), (7, 32), (1, 5), (31, 32)):
        imgs = rng.integers(0, 256, (12, s, s), dtype=np.uint8)
        imgs[0], imgs[1] = 255, 0
        want = np.stack([np.array(Image.fromarray(i).resize((o, o), Image.BILINEAR)) for i in imgs])
        assert np.array_equal(mnist.resize_u8(imgs, o), want), (s, o)


def test_sampler_and_host_compose_reproduce_the_reference_clips(fixture):
    T, seed = int(fixture["T"]), int(fixture["seed"])
    for split in ("train", "test"):
        sprites = fixture[f"{split}/sprites"]
        for nd, size in fixture["combos"].tolist():
            want = fixture[f"{split}/{nd}x{size}/crc"].tolist()
            ids, pos = mnist.MovingMnistSampler(len(sprites), T, nd, size, seed).draw(len(want))
            assert ids.dtype == np.int32 and ids.shape == (len(want), nd)
            assert pos.dtype == np.int32 and pos.shape == (len(want), nd, T, 2)
            assert pos.min() >= 0 and pos.max() <= size - mnist.DIGIT_SIZE
            clips = mnist.compose_host(sprites, ids, pos, size)
            assert np.array_equal(clips[0], fixture[f"{split}/{nd}x{size}/clip0"])
            assert [zlib.crc32(c.tobytes()) for c in clips] == want, (split, nd, size)


def test_batches_continue_the_stream_of_single_draws(fixture):
    """draw(B) twice == draw(2 B) once: a batch is B consecutive clips of the one stream."""
    a = mnist.MovingMnistSampler(48, 8, 2, 64, 5)
    b = mnist.MovingMnistSampler(48, 8, 2, 64, 5)
    one = b.draw(6)
    two = [a.draw(3), a.draw(3)]
    assert np.array_equal(np.concatenate([t[0] for t in two]), one[0])
    assert np.array_equal(np.concatenate([t[1] for t in two]), one[1])
    det = mnist.MovingMnistSampler(48, 30, 2, 64, 5, deterministic=True).draw(4)[1]
    assert det.min() >= 0 and det.max() <= 32
    with pytest.raises(SystemExit, match="no room"):
        mnist.MovingMnistSampler(48, 8, 2, 32, 5)


def test_recorded_clip0_holds_clipped_and_unclipped_sums_of_digits(fixture):
    """The fixture exercises both branches of `x[x > 1] = 1` where digits overlap."""
    T, seed = int(fixture["T"]), int(fixture["seed"])
    for split in ("train", "test"):
        sprites = fixture[f"{split}/sprites"]
        f = sprites.astype(np.float32) / np.float32(255)
        ids, pos = mnist.MovingMnistSampler(len(sprites), T, 2, 64, seed).draw(1)
        total, hits = np.zeros((T, 64, 64), np.float32), np.zeros((T, 64, 64), np.int32)
        for n in range(2):
            for t in range(T):
                sy, sx = pos[0, n, t]
                total[t, sy:sy + 32, sx:sx + 32] += f[ids[0, n]]
                hits[t, sy:sy + 32, sx:sx + 32] += f[ids[0, n]] > 0
        clip0 = fixture[f"{split}/2x64/clip0"][..., 0]
        both = hits >= 2
        assert (both & (total > 1)).any() and (both & (total < 1) & (total > 0)).any()
        assert np.array_equal(clip0, np.minimum(total, np.float32(1)))


def _opt(root):
    return types.SimpleNamespace(dataset="smmnist", data_root=root, image_width=64, channels=1, local_batch=3, rank=0,
                                 num_digits=2, synthetic_data=False)


def test_without_mnist_files_the_host_half_is_todays_generator(tmp_path, capsys, monkeypatch):
    """No MNIST files: make_batch_generator draws what SyntheticMovingMNIST(seed).trajectories draws, warns with today's text,
    and - for an existing directory - lists the paths it tried."""
    drawn = []
    monkeypatch.setattr(data.SyntheticMovingMNIST, "compose_device", lambda self, ids, pos, device: drawn.append((ids, pos)))
    warning = ("WARNING: synthetic data - Moving-MNIST trajectories over synthetic sprites (not MNIST digits); --data_root is "
               "ignored\n")
    for root, listed in ((str(tmp_path), True), (os.path.join(str(tmp_path), "nowhere"), False), ("path/to/data/", False)):
        del drawn[:]
        gen = data.make_batch_generator(_opt(root), 7, 21, device="cpu")
        for _ in range(2):
            next(gen)()
        ref = data.SyntheticMovingMNIST(seq_len=7, num_digits=2, image_size=64, seed=21)
        for ids, pos in drawn:
            want = ref.trajectories(3)
            assert np.array_equal(ids, want[0]) and np.array_equal(pos, want[1])
        err = capsys.readouterr().err
        assert err.startswith(warning)
        rest = err[len(warning):]
        if listed:
            assert rest.count("\n") == 1 and all(p in rest for p in mnist.candidates(root, True) + mnist.candidates(root, False))
        else:
            assert rest == ""


def test_half_a_tree_is_not_a_tree(tmp_path, capsys, monkeypatch):
    """Only the train file: torchvision would download the rest; here it is the synthetic fallback, and it says what it missed."""
    monkeypatch.setattr(data.SyntheticMovingMNIST, "compose_device", lambda self, ids, pos, device: None)
    mnist_tree.write(os.path.join(str(tmp_path), "raw"), True, mnist_tree.images(0, True), gz=False)
    next(data.make_batch_generator(_opt(str(tmp_path)), 7, 21, device="cpu"))()
    err = capsys.readouterr().err
    assert "synthetic data" in err and "t10k-images-idx3-ubyte" in err


def test_synthetic_data_flag_keeps_the_sprites_even_with_a_tree(tree, capsys, monkeypatch):
    monkeypatch.setattr(data.SyntheticMovingMNIST, "compose_device", lambda self, ids, pos, device: None)
    opt = _opt(tree)
    opt.synthetic_data = True
    next(data.make_batch_generator(opt, 7, 21, device="cpu"))()
    err = capsys.readouterr().err
    assert "synthetic data" in err and "tried" not in err


def test_op_wrappers_refuse_host_tensors():
    import torch
    from dvg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mnist_scale_u8(torch.zeros(2, 28, 28, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moving_mnist_compose_u8(torch.zeros(2, 32, 32, dtype=torch.uint8), np.zeros((1, 2), np.int32),
                                    np.zeros((1, 2, 4, 2), np.int32), 4, 64)


def test_kernel_entry_points_check_their_arguments_on_the_host():
    """Fake pointers, never dereferenced: the checks fire before any launch."""
    import ctypes
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    assert lib.dvg_mnist_scale_u8(one, one, 4, 32, 28, one, one, None) == 1 and b"up-scaling" in lib.dvg_last_error()
    assert lib.dvg_mnist_scale_u8(one, one, 4, 28, 128, one, one, None) == 1
    assert lib.dvg_mnist_scale_u8(one, one, 0, 28, 32, one, one, None) == 1
    assert lib.dvg_mnist_scale_u8(one, None, 4, 28, 32, one, one, None) == 2
    assert lib.dvg_moving_mnist_compose_u8(one, one, one, one, 8, 4, 2, 2, 30, 32, None) == 1          # canvas < digit
    assert lib.dvg_moving_mnist_compose_u8(one, one, one, one, 8, 4, 2, 2, 66, 32, None) == 1 and b"multiple of 4" in lib.dvg_last_error()
    assert lib.dvg_moving_mnist_compose_u8(one, one, None, one, 8, 4, 2, 2, 64, 32, None) == 2
