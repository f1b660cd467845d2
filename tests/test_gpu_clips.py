"""GPU: dvg_clip_gather_u8 against the reference's host path (imread / 255. + utils.normalize_data), and the KTH / UCF / BAIR
pipeline end to end - make_batch_generator, train.py and generate_frames.py on the tree of tests/clip_tree.py, pinned by what
the reference's loaders returned on it (tests/golden/reference_clips.npz)."""
import gzip
import io
import os
import re
import types
import zlib

import numpy as np
import pytest
import torch

from dvg_amd import datasets, ops, utils
from dvg_amd.data import make_batch_generator
from tests import clip_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_clips.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture):
    return clip_tree.build(tmp_path_factory.mktemp("clips"), int(fixture["tree_seed"]))


def reference_batch(pool, first, T, C):
    """What the reference hands the model: per clip imread(f) / 255. in float64 (channel 0 for KTH), stacked to (B,T,H,W,C),
    through utils.normalize_data -> T x (B,C,H,W) float32."""
    x = np.stack([pool[f:f + T, :, :, :C] for f in first])
    opt = types.SimpleNamespace(dataset="kth")
    seq, _ = utils.normalize_data(opt, torch.FloatTensor, (torch.from_numpy(x / 255.), torch.zeros(len(first))))
    return torch.stack(seq)


@pytest.mark.parametrize("C,pool_c", [(1, 1), (1, 3), (3, 3)])
@pytest.mark.parametrize("size", [64, 128])
def test_clip_gather_is_bit_equal_to_the_reference_host_path(C, pool_c, size):
    rng = np.random.default_rng(size + 10 * C + pool_c)
    n = 41
    pool = rng.integers(0, 256, (n, size, size, pool_c), dtype=np.uint8)
    pool[0, 0, :, 0] = np.arange(size) % 256                      # every byte value is in the pool
    pool[1] = np.arange(size * size * pool_c, dtype=np.int64).reshape(size, size, pool_c) % 256
    dpool = torch.from_numpy(pool).to(DEV)
    for B in (1, 5, 64):
        for T in (1, 12, 20):
            first = rng.integers(0, n - T + 1, B).astype(np.int64)
            first[0], first[-1] = n - T, 0                          # the last and the first pool positions
            got = ops.clip_gather(dpool, first, T, C)
            assert got.shape == (T, B, C, size, size) and got.dtype == torch.float32 and got.is_contiguous()
            want = reference_batch(pool, first, T, C)
            assert torch.equal(got.cpu(), want), (B, T, float((got.cpu() - want).abs().max()))


def test_clip_gather_frames_that_are_no_multiple_of_the_tile_and_a_device_index():
    """24 x 48 = 1152 pixels: the second 1024-pixel tile of every frame is partial; `first` on the device is clamped."""
    rng = np.random.default_rng(5)
    for pool_c, C in ((1, 1), (3, 1), (3, 3)):
        pool = rng.integers(0, 256, (9, 24, 48, pool_c), dtype=np.uint8)
        dpool = torch.from_numpy(pool).to(DEV)
        first = np.array([3, 0, 5], np.int64)
        got = ops.clip_gather(dpool, first, 4, C)
        assert torch.equal(got.cpu(), reference_batch(pool, first, 4, C))
        wild = torch.tensor([-4, 2, 10 ** 12], dtype=torch.int64, device=DEV)          # device data: clamped to [0, n - T]
        got = ops.clip_gather(dpool, wild, 4, C)
        assert torch.equal(got.cpu(), reference_batch(pool, np.array([0, 2, 5]), 4, C))


def test_clip_gather_rejects_an_out_of_range_first_on_the_host():
    dpool = torch.zeros(10, 64, 64, 1, dtype=torch.uint8, device=DEV)
    for bad in ([0, 7], [-1, 2], [10]):
        with pytest.raises(RuntimeError, match="leave the pool"):
            ops.clip_gather(dpool, np.array(bad, np.int64), 4, 1)
    assert ops.clip_gather(dpool, np.array([0, 6], np.int64), 4, 1).shape == (4, 2, 1, 64, 64)
    with pytest.raises(RuntimeError, match="int64"):
        ops.clip_gather(dpool, np.array([0, 1], np.int32), 4, 1)
    with pytest.raises(RuntimeError, match="pool of 1 channels"):
        ops.clip_gather(dpool, np.array([0], np.int64), 4, 3)


@pytest.mark.parametrize("dataset", ["kth", "ucf", "bair"])
@pytest.mark.parametrize("split", ["train", "test"])
def test_make_batch_generator_reproduces_the_reference_draws(tree, fixture, dataset, split, capsys):
    T, seed = int(fixture["T"]), int(fixture["seed"])
    want = fixture[f"{dataset}/{split}/crc"].tolist()
    B = 8
    opt = types.SimpleNamespace(dataset=dataset, data_root=clip_tree.data_root(tree, dataset), image_width=64,
                                channels=1 if dataset == "kth" else 3, local_batch=B, rank=0, data_threads=5,
                                synthetic_data=False)
    gen = make_batch_generator(opt, T, seed, torch.device(DEV), train=split == "train")
    crcs = []
    for k in range(len(want) // B):
        x = next(gen)()
        assert len(x) == T and tuple(x[0].shape) == (B, opt.channels, 64, 64)
        clips = torch.stack(x).permute(1, 0, 3, 4, 2).contiguous().cpu().numpy()          # (B,T,H,W,C)
        if k == 0:
            assert np.array_equal(clips[0], fixture[f"{dataset}/{split}/clip0"])
        crcs += [zlib.crc32(c.tobytes()) for c in clips]
    assert crcs == want
    assert "synthetic" not in capsys.readouterr().err


def _losses(out):
    rows = re.findall(r"\[\d+\] mse loss: (\S+) \(\d+\) (\S+)", out)
    assert rows
    return [float(v) for r in rows for v in r]


@pytest.mark.parametrize("dataset,channels", [("kth", 1), ("bair", 3)])
@pytest.mark.parametrize("graphed", [True, False])
def test_train_runs_on_a_dataset_tree(tree, tmp_path, capsys, dataset, channels, graphed):
    import train
    train.main(["--model", "dcgan", "--batch_size", "4", "--n_past", "2", "--n_future", "3", "--n_eval", "6", "--niter", "1",
                "--epoch_size", "2", "--no_images", "--dataset", dataset, "--channels", str(channels), "--data_root",
                clip_tree.data_root(tree, dataset), "--output_path", str(tmp_path)] + ([] if graphed else ["--no_hip_graph"]))
    cap = capsys.readouterr()
    assert all(np.isfinite(v) for v in _losses(cap.out)), cap.out
    assert "synthetic" not in cap.err
    sample = torch.load(os.path.join(str(tmp_path), "sample_0.pt"))
    assert bool(torch.isfinite(sample["gen"]).all())


def test_generate_frames_evaluates_on_the_test_split(tree, tmp_path, fixture):
    """The reference-format checkpoint fixture (dataset kth) with --data_root <tree>: the conditioning frames of the saved
    posterior rollout are the first n_past frames of the first clip make_batch_generator draws from the TEST split."""
    import generate_frames
    from oracle import params
    raw = gzip.open(os.path.join(ROOT, "tests", "golden", "reference_checkpoint_zeroed.pth.gz")).read()
    ck = torch.load(io.BytesIO(raw), map_location="cpu", weights_only=False)
    ck["encoder"].load_state_dict(params.fill_state_dict(ck["encoder"].state_dict(), 120))
    ck["decoder"].load_state_dict(params.fill_state_dict(ck["decoder"].state_dict(), 121,
                                                         params.decoder_transposed_keys(ck["decoder"].state_dict(), "dcgan")))
    ck["frame_predictor"].load_state_dict(params.fill_state_dict(ck["frame_predictor"].state_dict(), 300))
    ck["gp_layer"], ck["likelihood"] = params.gp_state(710)
    n_past, seed = ck["opt"].n_past, ck["opt"].seed
    torch.save(ck, os.path.join(str(tmp_path), "kth.pth"))
    root = clip_tree.data_root(tree, "kth")
    generate_frames.main(["--model_dir", str(tmp_path), "--dataset", "kth", "--data_root", root, "--batch_size", "4",
                          "--n_eval", "12", "--n_future", "7", "--nsample", "2", "--nbatches", "1", "--no_images",
                          "--log_dir", str(tmp_path) + "/logs"])
    res = torch.load(os.path.join(str(tmp_path), "logs", "gen", "sample_lstm_0.pt"))
    assert res["psnr"].shape == (4, 2, 12 - n_past) and bool(torch.isfinite(res["psnr"]).all())
    assert bool(torch.isfinite(res["ssim"]).all())
    index = datasets.open_index("kth", root, False)
    pool = datasets.build_pool(index, 64, None)
    first, _ = datasets.make_sampler(index, 12, generate_frames.data_seed(seed)).draw()
    want = torch.from_numpy((pool[first:first + n_past].numpy()[..., :1] / 255.).astype(np.float32)).permute(0, 3, 1, 2)
    assert torch.equal(res["posterior"][:n_past], want)
    train_index = datasets.open_index("kth", root, True)
    assert not any(f in set(sum(train_index.sequences, [])) for f in index.sequences[0])
