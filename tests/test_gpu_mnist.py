"""GPU: Moving-MNIST from real digits - dvg_mnist_scale_u8 against Pillow's output, dvg_moving_mnist_compose_u8 against the
host compositing, and make_batch_generator, train.py and generate_frames.py on the tree of tests/mnist_tree.py, pinned by what
the reference's data/moving_mnist.py returned on it (tests/golden/reference_mnist.npz).  Every comparison is bit-exact."""
import contextlib
import io
import os
import re
import types
import zlib

import numpy as np
import pytest
import torch

from dvg_amd import mnist, ops
from dvg_amd.data import make_batch_generator
from tests import mnist_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TRAIN_ARGS = ["--model", "dcgan", "--batch_size", "4", "--n_past", "2", "--n_future", "3", "--n_eval", "6", "--niter", "1",
              "--epoch_size", "2", "--no_images", "--dataset", "smmnist"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_mnist.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture):
    return mnist_tree.build(tmp_path_factory.mktemp("mnist"), int(fixture["tree_seed"]))


@pytest.fixture(scope="module")
def digits(fixture):
    """(raw 28x28, Pillow's 32x32) of all 72 digits of the tree."""
    seed = int(fixture["tree_seed"])
    return (np.concatenate([mnist_tree.images(seed, True), mnist_tree.images(seed, False)]),
            np.concatenate([fixture["train/sprites"], fixture["test/sprites"]]))


@pytest.mark.parametrize("n", [72, 1, 5])
def test_scale_equals_pillow(digits, n):
    """n = 5: the second workgroup holds one digit of its four; n = 1: a single partial workgroup."""
    raw, want = digits
    got = ops.mnist_scale_u8(torch.from_numpy(raw[-n:].copy()).to(DEV), 32)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 32, 32) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want[-n:])


def test_scale_with_equal_sizes_is_the_identity(digits):
    want = digits[1][:7]
    assert np.array_equal(ops.mnist_scale_u8(torch.from_numpy(want.copy()).to(DEV), 32).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="up-scaling"):
        ops.mnist_scale_u8(torch.from_numpy(want.copy()).to(DEV), 28)


def _compose_case(name, sprites):
    """(ids, pos, T, S) of one case; positions are (sy, sx)."""
    n = len(sprites)
    if name in ("3x5x3x64", "1x2x2x128"):
        B, T, ND, S = (int(v) for v in name.split("x"))
        return mnist.MovingMnistSampler(n, T, ND, S, 77).draw(B) + (T, S)
    if name == "corners":                       # the first and the last position a trajectory takes, in every combination
        lo, hi = 0, 64 - 32 - 1
        pos = np.array([[[[lo, lo], [hi, hi], [lo, hi], [hi, lo]], [[hi, hi], [lo, lo], [hi, lo], [lo, hi]]]], np.int32)
        return np.array([[3, 5]], np.int32), pos, 4, 64
    if name == "same-position":                 # two digits on top of each other: sums up to 2, clipped; a digit on itself
        pos = np.array([[[[7, 9], [0, 0]], [[7, 9], [0, 0]]], [[[20, 1], [31, 31]], [[20, 1], [31, 31]]]], np.int32)
        return np.array([[0, 1], [6, 6]], np.int32), pos, 2, 64
    assert name == "one-digit"
    ids = np.array([[5], [n - 1], [0]], np.int32)                               # 5 = a full-range noise digit
    pos = np.array([[[[0, 0], [3, 30], [32, 1]]], [[[31, 31], [16, 17], [1, 2]]], [[[5, 5], [5, 6], [5, 7]]]], np.int32)
    return ids, pos, 3, 64


@pytest.mark.parametrize("case", ["3x5x3x64", "1x2x2x128", "corners", "same-position", "one-digit"])
def test_compose_u8_equals_the_host_compose_and_the_float_kernel(digits, case):
    sprites = digits[1]
    ids, pos, T, S = _compose_case(case, sprites)
    B = len(ids)
    dsprites = torch.from_numpy(sprites).to(DEV)
    got = ops.moving_mnist_compose_u8(dsprites, ids, pos, T, S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, B, 1, S, S) and got.is_contiguous()
    want = torch.from_numpy(mnist.compose_host(sprites, ids, pos, S)).permute(1, 0, 4, 2, 3)      # (B,T,S,S,1) -> (T,B,1,S,S)
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    if case == "same-position":
        assert float(want.max()) == 1.0 and bool(((want > 0) & (want < 1)).any())
    dids, dpos = torch.from_numpy(ids).to(DEV), torch.from_numpy(pos).to(DEV)
    assert torch.equal(ops.moving_mnist_compose_u8(dsprites, dids, dpos, T, S), got)               # device ids / pos
    # the float pool is divided on the HOST, an IEEE division like ToTensor's: torch's device kernel for tensor / scalar
    # multiplies by the reciprocal, which is another float32 for 126 of the 256 bytes
    fsprites = (torch.from_numpy(sprites).float() / 255).to(DEV)
    assert torch.equal(ops.moving_mnist_compose(fsprites, dids, dpos, T, S), got)


def test_compose_u8_checks_host_positions_and_clamps_device_ids(digits):
    sprites = digits[1]
    dsprites = torch.from_numpy(sprites).to(DEV)
    ids, pos = np.array([[0, 1]], np.int32), np.zeros((1, 2, 2, 2), np.int32)
    for bad in (33, -1):
        p = pos.copy()
        p[0, 1, 1, 0] = bad
        with pytest.raises(RuntimeError, match="leave the canvas"):
            ops.moving_mnist_compose_u8(dsprites, ids, p, 2, 64)
    with pytest.raises(RuntimeError, match="outside the pool"):
        ops.moving_mnist_compose_u8(dsprites, np.array([[0, len(sprites)]], np.int32), pos, 2, 64)
    with pytest.raises(RuntimeError, match="int32"):
        ops.moving_mnist_compose_u8(dsprites, ids.astype(np.int64), pos, 2, 64)
    pos[0, :, :, :] = 32                                                        # S - D itself is a legal position
    assert ops.moving_mnist_compose_u8(dsprites, ids, pos, 2, 64).shape == (2, 1, 1, 64, 64)
    wild = torch.tensor([[-5, 10 ** 6]], dtype=torch.int32, device=DEV)         # device data: clamped to the pool
    got = ops.moving_mnist_compose_u8(dsprites, wild, torch.from_numpy(pos).to(DEV), 2, 64)
    want = ops.moving_mnist_compose_u8(dsprites, np.array([[0, len(sprites) - 1]], np.int32), pos, 2, 64)
    assert torch.equal(got, want)


@pytest.mark.parametrize("split", ["train", "test"])
def test_make_batch_generator_reproduces_the_reference_clips(tree, fixture, split, capsys):
    T, seed = int(fixture["T"]), int(fixture["seed"])
    B = 8
    for nd, size in fixture["combos"].tolist():
        want = fixture[f"{split}/{nd}x{size}/crc"].tolist()
        opt = types.SimpleNamespace(dataset="smmnist", data_root=tree, image_width=size, channels=1, local_batch=B, rank=0,
                                    num_digits=nd, synthetic_data=False)
        gen = make_batch_generator(opt, T, seed, torch.device(DEV), train=split == "train")
        crcs = []
        for k in range(len(want) // B):
            x = next(gen)()
            assert len(x) == T and tuple(x[0].shape) == (B, 1, size, size)
            clips = torch.stack(x).permute(1, 0, 3, 4, 2).contiguous().cpu().numpy()          # (B,T,H,W,1)
            if k == 0:
                assert np.array_equal(clips[0], fixture[f"{split}/{nd}x{size}/clip0"])
            crcs += [zlib.crc32(c.tobytes()) for c in clips]
        assert crcs == want, (nd, size)
    cap = capsys.readouterr()
    assert "synthetic" not in cap.err and "synthetic" not in cap.out


def _losses(out):
    rows = re.findall(r"\[\d+\] mse loss: (\S+) \(\d+\) (\S+)", out)
    assert rows
    return [float(v) for r in rows for v in r]


def _train(extra, out_dir):
    import train
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        train.main(TRAIN_ARGS + ["--output_path", str(out_dir)] + extra)
    return out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def trained(tree, tmp_path_factory):
    """One epoch of two graphed iterations on the tree: (directory with model.pth, stdout, stderr)."""
    d = tmp_path_factory.mktemp("trained")
    return (str(d),) + _train(["--data_root", tree], d)


def _check_training(out_dir, out, err):
    assert all(np.isfinite(v) for v in _losses(out)), out
    sample = torch.load(os.path.join(out_dir, "sample_0.pt"))
    assert bool(torch.isfinite(sample["gen"]).all())


def test_train_runs_on_the_tree_graphed(trained):
    out_dir, out, err = trained
    _check_training(out_dir, out, err)
    assert "synthetic" not in err


def test_train_runs_on_the_tree_without_hip_graph(tree, tmp_path):
    out, err = _train(["--data_root", tree, "--no_hip_graph"], tmp_path)
    _check_training(str(tmp_path), out, err)
    assert "synthetic" not in err


def test_generate_frames_evaluates_on_the_test_digits(tree, trained, tmp_path, fixture, capsys):
    """train.py's checkpoint with --data_root <tree>: the conditioning frames of the saved posterior rollout are the first
    n_past frames of the first clip of the TEST split, drawn as the reference draws it."""
    import generate_frames
    generate_frames.main(["--model_dir", trained[0], "--dataset", "smmnist", "--data_root", tree, "--batch_size", "4",
                          "--n_eval", "8", "--n_future", "6", "--nsample", "2", "--nbatches", "1", "--no_images",
                          "--log_dir", str(tmp_path) + "/logs"])
    assert "synthetic" not in capsys.readouterr().err
    res = torch.load(os.path.join(str(tmp_path), "logs", "gen", "sample_lstm_0.pt"))
    assert res["psnr"].shape == (4, 2, 6) and bool(torch.isfinite(res["psnr"]).all())
    assert bool(torch.isfinite(res["ssim"]).all())
    assert generate_frames.data_seed(1) == int(fixture["seed"]) and int(fixture["T"]) == 8      # the fixture's own stream
    want = torch.from_numpy(fixture["test/2x64/clip0"]).permute(0, 3, 1, 2)                        # (T,1,S,S)
    assert torch.equal(res["posterior"][:2], want[:2])


def test_train_without_data_root_still_warns_and_trains_on_the_sprites(tmp_path):
    out, err = _train([], tmp_path)
    _check_training(str(tmp_path), out, err)
    assert "WARNING: synthetic data - Moving-MNIST trajectories over synthetic sprites (not MNIST digits); --data_root is " \
           "ignored" in err
    assert "tried" not in err
