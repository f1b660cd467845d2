"""GPU: `--dataset frames --resize FILTER` end to end on the tree of tests/frames_tree.py - the device pool against the host
pool (Pillow itself), the batches of make_batch_generator against Pillow-resized bytes / 255, `--augment` on top, and
generate_frames.py / train.py on off-size frames."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

from dvg_amd import datasets  # noqa: E402
from dvg_amd.data import make_batch_generator  # noqa: E402
from tests import frames_tree  # noqa: E402
from tests.augment_ref import reference_aug_batch  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S, B, T = 64, 2, 4


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return frames_tree.build(tmp_path_factory.mktemp("frames"))


@pytest.fixture(scope="module")
def host_pools(tree):
    """Per split: the index and the Pillow-resized pool (bilinear, crop), computed once and left unchanged."""
    out = {}
    for train in (True, False):
        index = datasets.open_index("frames", tree, train)
        out[train] = (index, frames_tree.pillow_pool(index, S, "bilinear", "crop"))
    return out


def _opt(tree, augment="", resize="bilinear", channels=3):
    return types.SimpleNamespace(dataset="frames", data_root=tree, image_width=S, channels=channels, local_batch=B, rank=0,
                                 data_threads=5, synthetic_data=False, augment=augment, resize=resize, resize_fit="crop")


@pytest.mark.parametrize("train", [True, False])
def test_device_pool_equals_the_host_pool_byte_for_byte(tree, host_pools, train, monkeypatch):
    index, want = host_pools[train]
    cpu = datasets.build_pool(index, S, None, resize=("bilinear", "crop"))
    assert np.array_equal(cpu.numpy(), want)
    gpu = datasets.build_pool(index, S, torch.device(DEV), resize=("bilinear", "crop"))
    assert gpu.is_cuda and np.array_equal(gpu.cpu().numpy(), want)
    if train:       # a staging buffer smaller than the tree: several chunks, a run cut in two, the same bytes; other filters
        monkeypatch.setattr(datasets, "STAGING_BYTES", 5 * 30 * 40 * 3 + 100)
        assert np.array_equal(datasets.build_pool(index, S, torch.device(DEV), threads=3, resize=("bilinear", "crop")).cpu().numpy(), want)
        for f, fit in (("lanczos", "stretch"), ("box", "crop")):
            got = datasets.build_pool(index, S, torch.device(DEV), resize=(f, fit)).cpu().numpy()
            assert np.array_equal(got, frames_tree.pillow_pool(index, S, f, fit)), (f, fit)
        with pytest.raises(SystemExit, match=r"is 40x30, not 64x64"):
            datasets.build_pool(index, S, torch.device(DEV))


@pytest.mark.parametrize("train", [True, False])
def test_batches_are_the_resized_bytes_over_255(tree, host_pools, train):
    index, pool = host_pools[train]
    seed = 21
    gen = make_batch_generator(_opt(tree), T, seed, torch.device(DEV), train=train)
    sampler = datasets.make_sampler(index, T, seed)
    for _ in range(5):
        first = [sampler.draw()[0] for _ in range(B)]
        x = next(gen)()
        assert len(x) == T and tuple(x[0].shape) == (B, 3, S, S)
        want = np.stack([pool[f:f + T] for f in first], 1).astype(np.float32) / np.float32(255)        # (T,B,H,W,C)
        assert np.array_equal(torch.stack(x).permute(0, 1, 3, 4, 2).cpu().numpy(), want)
    one = next(make_batch_generator(_opt(tree, channels=1), T, seed, torch.device(DEV), train=train))()    # --channels 1: channel 0
    assert tuple(one[0].shape) == (B, 1, S, S)


def test_augment_applies_to_the_resized_pool(tree, host_pools):
    index, pool = host_pools[True]
    seed, spec = 8, "hflip"
    gen = make_batch_generator(_opt(tree, augment=spec), T, seed, torch.device(DEV))
    sampler = datasets.make_sampler(index, T, seed)
    twin = datasets.ClipAugmenter(spec, seed ^ datasets.AUGMENT_SEED_XOR)
    flipped = False
    for _ in range(6):
        first = np.array([sampler.draw()[0] for _ in range(B)], np.int64)
        geom, photo = twin.draw(B)
        assert torch.equal(torch.stack(next(gen)()).cpu(), reference_aug_batch(pool, first, geom, photo, T, 3))
        flipped |= bool(geom[:, 0].any())
    assert flipped


def test_generate_frames_runs_on_a_frames_tree(tree, tmp_path):
    """A fresh process, under its own time limit: generate_frames.py on the test split of off-size frames."""
    logs = str(tmp_path / "logs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_frames.py"), "--synthetic_ckpt", "--dataset", "frames", "--data_root",
                        tree, "--resize", "bicubic", "--channels", "3", "--batch_size", "2", "--n_past", "2", "--n_future", "2",
                        "--n_eval", "4", "--nsample", "2", "--nbatches", "1", "--no_images", "--log_dir", logs],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    res = torch.load(os.path.join(logs, "gen", "sample_lstm_0.pt"))
    assert res["psnr"].shape == (2, 2, 2) and bool(torch.isfinite(res["psnr"]).all()) and bool(torch.isfinite(res["ssim"]).all())
    index = datasets.open_index("frames", tree, False)
    want = frames_tree.pillow_pool(index, S, "bicubic", "crop")[:2].astype(np.float32) / np.float32(255)    # clip x, frames 0 and 1
    assert np.array_equal(res["posterior"][:2].numpy(), want.transpose(0, 3, 1, 2))                          # the conditioning frames


def test_train_runs_with_the_flag_and_exits_without_it(tree, tmp_path, capsys):
    import train
    args = ["--model", "dcgan", "--dataset", "frames", "--channels", "3", "--data_root", tree, "--batch_size", "2", "--n_past", "2",
            "--n_future", "2", "--n_eval", "4", "--niter", "1", "--epoch_size", "2", "--no_images", "--no_save", "--output_path", str(tmp_path)]
    with pytest.raises(SystemExit, match=r"is 40x30, not 64x64"):
        train.main(args + ["--resize", "none"])
    capsys.readouterr()
    train.main(args + ["--resize", "bilinear"])
    out = capsys.readouterr()
    assert "mse loss" in out.out and "synthetic" not in out.err
