"""GPU: dvg_clip_gather_aug_u8 against its numpy statement (tests/augment_ref.py), bit for bit - every transform alone and all
together, the clamps of device-resident parameters - then `--augment` through make_batch_generator and through train.py with a
resume.  Shapes: 64x64 (whole tiles of 16 rows), 24x48 (21 rows per tile: a partial last tile, rows of 48 and 144 bytes) and
128x128 (8 rows per tile), each for (pool_c, C) = (1,1), (3,1), (3,3); T = 4, B = 5."""
import os
import types
import zlib

import numpy as np
import pytest
import torch

from dvg_amd import datasets, ops
from dvg_amd.data import make_batch_generator
from tests import clip_tree
from tests.augment_ref import reference_aug_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
T, B, N = 4, 5, 11
SIZES = [(64, 64), (24, 48), (128, 128)]
CHANNELS = [(1, 1), (3, 1), (3, 3)]
FIRST = np.array([N - T, 0, 3, 5, 2], np.int64)            # clip 0 ends at the pool's last frame, clip 1 starts at its first
IDENT_G = np.zeros((B, 4), np.int32)
IDENT_P = np.tile(np.float32([1.0, 0.0]), (B, 1))


def _geom(hflip=0, reverse=0, dy=0, dx=0):
    g = np.zeros((B, 4), np.int32)
    for col, v in enumerate((hflip, reverse, dy, dx)):
        g[:, col] = v
    return g


# gain / bias: saturates at 1 only; at 0 only (1.5 v - 0.9 <= 0.6); neither (within [0.1, 0.9]); both ends; the identity
PHOTO = np.float32([[2.0, 0.3], [1.5, -0.9], [0.8, 0.1], [1.4, -0.2], [1.0, 0.0]])
CASES = {
    "hflip": (_geom(hflip=[1, 0, 1, 1, 0]), IDENT_P),
    "reverse": (_geom(reverse=[1, 1, 0, 1, 0]), IDENT_P),             # on the clip that starts at n - T and on the one at 0
    "dx_odd": (_geom(dx=[1, 2, 3, 5, -7]), IDENT_P),                  # no multiples of 4
    "dx_limit": (_geom(dx=[16, -16, 4, -1, 8]), IDENT_P),
    "dy": (_geom(dy=[1, -3, 16, -16, 0]), IDENT_P),
    "hflip_dx": (_geom(hflip=1, dx=[3, -5, 16, -16, 1]), IDENT_P),    # flip with a positive and with a negative shift
    "photo": (IDENT_G, PHOTO),
    "all": (_geom(hflip=[1, 1, 0, 1, 0], reverse=[1, 0, 1, 1, 0], dy=[-3, 16, 1, -16, 2], dx=[5, -7, 16, 3, -16]), PHOTO),
}


def _pool(size, pool_c):
    h, w = size
    rng = np.random.default_rng(h * 1000 + w + pool_c)
    pool = rng.integers(0, 256, (N, h, w, pool_c), dtype=np.uint8)
    pool[4] = (np.arange(h * w * pool_c, dtype=np.int64) % 256).reshape(h, w, pool_c)                  # every byte value
    pool[6] = ((np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(pool_c) * 85) % 256)   # a ramp
    return pool


@pytest.fixture(scope="module")
def pools():
    """(size, pool_c) -> (host pool, device pool), made once."""
    out = {}
    for size in SIZES:
        for pc in (1, 3):
            p = _pool(size, pc)
            out[size, pc] = (p, torch.from_numpy(p).to(DEV))
    return out


@pytest.mark.parametrize("pool_c,C", CHANNELS)
@pytest.mark.parametrize("size", SIZES)
def test_identity_parameters_give_the_plain_gathers_bits(pools, size, pool_c, C):
    pool, dpool = pools[size, pool_c]
    got = ops.clip_gather_aug(dpool, FIRST, IDENT_G, IDENT_P, T, C)
    assert got.shape == (T, B, C) + size and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, ops.clip_gather(dpool, FIRST, T, C))
    assert torch.equal(got.cpu(), reference_aug_batch(pool, FIRST, IDENT_G, IDENT_P, T, C))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("pool_c,C", CHANNELS)
@pytest.mark.parametrize("size", SIZES)
def test_every_transform_is_bit_equal_to_the_numpy_statement(pools, size, pool_c, C, case):
    pool, dpool = pools[size, pool_c]
    geom, photo = CASES[case]
    got = ops.clip_gather_aug(dpool, FIRST, geom, photo, T, C).cpu()
    want = reference_aug_batch(pool, FIRST, geom, photo, T, C)
    assert torch.equal(got, want), (case, float((got - want).abs().max()))
    plain = reference_aug_batch(pool, FIRST, IDENT_G, IDENT_P, T, C)
    assert not torch.equal(want, plain)                      # the case does something: the comparison can fail


def test_the_photometric_cases_saturate_where_they_say(pools):
    pool, _ = pools[(64, 64), 1]
    out = reference_aug_batch(pool, FIRST, IDENT_G, PHOTO, T, 1)
    lo, hi = [bool((out[:, b] == 0).any()) for b in range(B)], [bool((out[:, b] == 1).any()) for b in range(B)]
    assert (lo[0], hi[0]) == (False, True) and (lo[1], hi[1]) == (True, False) and (lo[2], hi[2]) == (False, False)
    assert (lo[3], hi[3]) == (True, True)


@pytest.mark.parametrize("pool_c,C", CHANNELS)
@pytest.mark.parametrize("size", SIZES)
def test_wild_device_parameters_are_clamped(pools, size, pool_c, C):
    """Device-resident parameters are never trusted: the result is the reference's at the clamped values."""
    pool, dpool = pools[size, pool_c]
    first = torch.tensor([-4, 2, 10 ** 12, 1, 0], dtype=torch.int64, device=DEV)
    geom = torch.tensor([[7, 0, 1000, -1000], [0, -3, -1000, 1000], [7, 1, 1000, 17], [0, 0, -17, 0], [1, 1, 0, 0]],
                        dtype=torch.int32, device=DEV)
    photo = torch.from_numpy(PHOTO).to(DEV)
    got = ops.clip_gather_aug(dpool, first, geom, photo, T, C).cpu()
    clamped = np.array([[1, 0, 16, -16], [0, 1, -16, 16], [1, 1, 16, 16], [0, 0, -16, 0], [1, 1, 0, 0]], np.int32)
    want = reference_aug_batch(pool, np.array([0, 2, N - T, 1, 0]), clamped, PHOTO, T, C)
    assert torch.equal(got, want)
    # host first with device geom / photo: the parts travel on their own
    got = ops.clip_gather_aug(dpool, FIRST, geom, photo, T, C).cpu()
    assert torch.equal(got, reference_aug_batch(pool, FIRST, clamped, PHOTO, T, C))


def test_the_op_refuses_bad_host_parameters():
    dpool = torch.zeros(N, 64, 64, 1, dtype=torch.uint8, device=DEV)
    for col, v in ((3, 17), (3, -17), (2, 17), (2, -2 ** 31)):
        g = IDENT_G.copy()
        g[2, col] = v
        with pytest.raises(RuntimeError, match="beyond"):
            ops.clip_gather_aug(dpool, FIRST, g, IDENT_P, T, 1)
    for v in (np.nan, np.inf):
        p = IDENT_P.copy()
        p[1, 0] = v
        with pytest.raises(RuntimeError, match="finite"):
            ops.clip_gather_aug(dpool, FIRST, IDENT_G, p, T, 1)
    with pytest.raises(RuntimeError, match="leave the pool"):
        ops.clip_gather_aug(dpool, np.array([0, N - T + 1], np.int64), IDENT_G[:2], IDENT_P[:2], T, 1)
    with pytest.raises(RuntimeError, match="int32"):
        ops.clip_gather_aug(dpool, FIRST, IDENT_G.astype(np.int64), IDENT_P, T, 1)
    with pytest.raises(RuntimeError, match=r"\(5,2\) float32"):
        ops.clip_gather_aug(dpool, FIRST, IDENT_G, torch.from_numpy(IDENT_P[:4]).to(DEV), T, 1)
    assert ops.clip_gather_aug(dpool, FIRST, IDENT_G, IDENT_P, T, 1).shape == (T, B, 1, 64, 64)


# ---- the generator ----------------------------------------------------------------------------------------------------------
SPEC = "hflip,reverse,shift=3,jitter=0.2"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_clips.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory, fixture):
    return clip_tree.build(tmp_path_factory.mktemp("clips"), int(fixture["tree_seed"]))


def _opt(tree, dataset, augment, batch=4):
    return types.SimpleNamespace(dataset=dataset, data_root=clip_tree.data_root(tree, dataset), image_width=64,
                                 channels=1 if dataset == "kth" else 3, local_batch=batch, rank=0, data_threads=5,
                                 synthetic_data=False, augment=augment)


@pytest.mark.parametrize("dataset", ["kth", "bair"])
def test_generator_augments_the_clips_the_plain_generator_draws(tree, dataset):
    """Six consecutive batches: reference_aug_batch on the host pool at the indices the sampler of the same seed draws, with the
    parameters a fresh ClipAugmenter of the derived seed draws; with identity parameters the same statement gives the plain
    generator's batches."""
    seq, seed, batch = 8, 13, 4
    opt = _opt(tree, dataset, SPEC, batch)
    aug = make_batch_generator(opt, seq, seed, torch.device(DEV))
    plain = make_batch_generator(_opt(tree, dataset, "", batch), seq, seed, torch.device(DEV))
    index = datasets.open_index(dataset, opt.data_root, True)
    pool = datasets.build_pool(index, 64, None).numpy()
    sampler = datasets.make_sampler(index, seq, seed)
    twin = datasets.ClipAugmenter(SPEC, seed ^ datasets.AUGMENT_SEED_XOR)
    seen = np.zeros(4, bool)
    for _ in range(6):
        first = np.array([sampler.draw()[0] for _ in range(batch)], np.int64)
        geom, photo = twin.draw(batch)
        got = torch.stack(next(aug)()).cpu()
        assert torch.equal(got, reference_aug_batch(pool, first, geom, photo, seq, opt.channels))
        ident = reference_aug_batch(pool, first, np.zeros((batch, 4), np.int32), np.tile(np.float32([1, 0]), (batch, 1)), seq,
                                    opt.channels)
        assert torch.equal(torch.stack(next(plain)()).cpu(), ident)
        seen |= (geom != 0).any(0)
    assert seen.all()                                          # every transform was drawn at least once


@pytest.mark.parametrize("dataset", ["kth", "bair"])
def test_test_split_generator_ignores_the_option(tree, fixture, dataset):
    seq, seed, batch = int(fixture["T"]), int(fixture["seed"]), 8
    want = fixture[f"{dataset}/test/crc"].tolist()
    gen = make_batch_generator(_opt(tree, dataset, SPEC, batch), seq, seed, torch.device(DEV), train=False)
    crcs = []
    for _ in range(len(want) // batch):
        clips = torch.stack(next(gen)()).permute(1, 0, 3, 4, 2).contiguous().cpu().numpy()          # (B,T,H,W,C)
        crcs += [zlib.crc32(c.tobytes()) for c in clips]
    assert crcs == want


# ---- train.py --augment, with a resume -----------------------------------------------------------------------------------------
def _checksum(out):
    lines = [ln for ln in out.splitlines() if "param checksum" in ln]
    assert len(lines) == 1, out
    return lines[0].split()[-2:]


@pytest.mark.parametrize("graphed", [True, False])
def test_train_augments_and_resumes_exactly(tree, tmp_path, capsys, graphed):
    """Two epochs in one run end with the checksum of one epoch + `--resume`; without the flag the run ends elsewhere; the state
    of an augmented run is refused by a run without the flag."""
    import train
    flag = ["--augment", "hflip,shift=2,jitter=0.1"]
    base = ["--model", "dcgan", "--dataset", "kth", "--channels", "1", "--data_root", clip_tree.data_root(tree, "kth"),
            "--batch_size", "4", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--epoch_size", "2", "--save_every", "1",
            "--no_images", "--print_param_checksum"] + ([] if graphed else ["--no_hip_graph"])
    whole, split, plain = (str(tmp_path / d) for d in ("whole", "split", "plain"))

    train.main(base + flag + ["--niter", "2", "--output_path", whole])
    out = capsys.readouterr().out
    assert "augment: hflip,shift=2,jitter=0.1 (train split only)\n" in out and "[01] mse loss" in out
    straight = _checksum(out)

    train.main(base + flag + ["--niter", "1", "--output_path", split])
    capsys.readouterr()
    train.main(base + flag + ["--niter", "2", "--output_path", split, "--resume", split])
    out = capsys.readouterr().out
    assert "resumed from" in out and out.count("mse loss") == 1 and "[01] mse loss" in out
    resumed = _checksum(out)
    print(f"\naugmented, {'hipGraph' if graphed else 'eager'}: two epochs {straight}, one + resume + one {resumed}")
    assert resumed == straight

    train.main(base + ["--niter", "2", "--output_path", plain])
    out = capsys.readouterr().out
    assert "augment:" not in out
    assert _checksum(out) != straight

    with pytest.raises(SystemExit) as e:
        train.main(base + ["--niter", "3", "--output_path", split, "--resume", split])
    assert str(e.value) == "data position: saved with --augment 'hflip,shift=2,jitter=0.1', this run has no --augment"
