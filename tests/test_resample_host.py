"""CPU: Pillow's 8-bit resampler restated on the host (dvg_amd/resample.py) against Pillow itself, byte for byte; the `frames`
index and sampler, the `--resize` options and the host pool of dvg_amd/datasets.py; dvg_resample_u8's argument checks."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from dvg_amd import datasets, mnist, resample  # noqa: E402
from tests import frames_tree, resample_cases  # noqa: E402


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return frames_tree.build(tmp_path_factory.mktemp("frames"))


# ---- the resampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", resample_cases.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_resize_u8_host_equals_pillow(geometry):
    H, W, S = geometry
    for C in (1, 3):
        for kind in resample_cases.KINDS:
            imgs = resample_cases.images(kind, 2, H, W, C)
            for box in resample_cases.boxes(H, W, S):
                for f in resample.FILTERS:
                    got = resample.resize_u8_host(imgs, (S, S), f, box)
                    assert got.dtype == np.uint8 and np.array_equal(got, resample_cases.pillow(imgs, S, f, box)), (C, kind, box, f)


def test_rectangular_targets_equal_pillow():
    imgs = resample_cases.images("random", 1, 50, 70, 3)
    for (h, w) in ((20, 33), (50, 16), (64, 70), (77, 90)):
        for f in ("box", "hamming", "lanczos"):
            want = np.asarray(Image.fromarray(imgs[0]).resize((w, h), resample.pil_filter(f)))
            assert np.array_equal(resample.resize_u8_host(imgs, (h, w), f)[0], want), (h, w, f)


def test_tables_restate_the_mnist_case_and_the_kernel_sizes():
    xmin, coef = resample.tables(28, 0, 28, 32, "bilinear")
    mmin, mcoef = mnist.resize_tables(28, 32)
    assert coef.shape == (32, 3) and np.array_equal(xmin, mmin)
    assert np.array_equal(coef, np.pad(mcoef, ((0, 0), (0, coef.shape[1] - mcoef.shape[1]))))
    assert np.array_equal(resample.resize_u8_host(resample_cases.images("random", 3, 28, 28, 1), (32, 32))[..., 0],
                          mnist.resize_u8(resample_cases.images("random", 3, 28, 28, 1)[..., 0], 32))
    # ksize = 2 * ceil(support * max(scale, 1)) + 1
    for f, in_size, out, k in (("box", 160, 64, 5), ("bilinear", 160, 64, 7), ("hamming", 7, 8, 3), ("bicubic", 320, 128, 11),
                               ("lanczos", 1000, 64, 95), ("lanczos", 5, 8, 7)):
        xmin, coef = resample.tables(in_size, 0, in_size, out, f)
        assert coef.shape == (out, k) and xmin.dtype == coef.dtype == np.int32
        assert xmin.min() >= 0 and (np.diff(xmin) >= 0).all() and xmin.max() < in_size
        assert (np.abs(coef.sum(1) - (1 << 22)) <= k).all()          # normalised, then rounded tap by tap
    assert resample.tables(100, 10, 90, 8, "bilinear")[0][0] >= 0 and resample.tables(100, 10, 90, 8, "bilinear")[0][0] < 20   # the box lives in xmin
    for bad in ((0, 0, 0, 4, "bilinear"), (8, 0, 9, 4, "bilinear"), (8, 4, 4, 4, "bilinear"), (8, 0, 8, 0, "bilinear"), (8, 0, 8, 4, "nearest")):
        with pytest.raises(ValueError):
            resample.tables(*bad)
    assert not resample.pass_needed(64, 0, 64, 64) and resample.pass_needed(64, 0, 48, 64) and resample.pass_needed(64, 1, 64, 64) \
        and resample.pass_needed(48, 0, 48, 64)


def test_fit_box():
    assert resample.fit_box(320, 240, 64, 64, "stretch") == (0, 0, 320, 240)
    assert resample.fit_box(320, 240, 64, 64, "crop") == (40, 0, 280, 240)           # landscape
    assert resample.fit_box(40, 1100, 64, 64, "crop") == (0, 530, 40, 570)           # portrait
    assert resample.fit_box(48, 48, 64, 64, "crop") == (0, 0, 48, 48)                # square
    assert resample.fit_box(65, 63, 64, 64, "crop") == (1, 0, 64, 63)                # odd: offset (W - m) // 2
    assert resample.fit_box(7, 5, 8, 8, "crop") == (1, 0, 6, 5)
    assert resample.fit_box(1, 1, 4, 4, "crop") == (0, 0, 1, 1)
    assert resample.fit_box(100, 100, 32, 16, "crop") == (0, 25, 100, 75)            # a 2:1 target
    assert resample.fit_box(300, 100, 32, 16, "crop") == (50, 0, 250, 100)
    with pytest.raises(ValueError):
        resample.fit_box(10, 10, 4, 4, "pad")


# ---- the frames index and sampler -------------------------------------------------------------------------------------------------
def test_frames_index_orders_and_separates(tree, tmp_path):
    train, test = datasets.open_index("frames", tree, True), datasets.open_index("frames", tree, False)
    rel = lambda idx: [[os.path.relpath(f, tree) for f in s] for s in idx.sequences]      # noqa: E731
    assert [os.path.dirname(s[0]) for s in rel(train)] == ["train/a", "train/b/deep", "train/c", "train/short"]    # sorted, nested, no `empty`
    assert [os.path.basename(f) for f in rel(train)[1]] == ["f%d.png" % k for k in range(12)]     # f2 before f10
    assert rel(train)[2][0].endswith(".jpg") and train.lengths.tolist() == [6, 12, 7, 2] and set(train.labels) == {-1}
    assert [os.path.dirname(s[0]) for s in rel(test)] == ["test/x", "test/y"] and test.split == "test"
    assert train.bases.tolist() == [0, 6, 18, 25] and train.n_frames == 27
    with pytest.raises(SystemExit, match="no_such"):
        datasets.open_index("frames", str(tmp_path / "no_such"), True)
    os.makedirs(tmp_path / "bare" / "train" / "nothing")
    with pytest.raises(SystemExit, match="no directory with"):
        datasets.open_index("frames", str(tmp_path / "bare"), True)
    # a tree that mixes L and RGB frames is refused when the pool is built
    mixed = tmp_path / "mixed"
    for clip, mode in (("a", "RGB"), ("b", "L")):
        os.makedirs(mixed / "train" / clip)
        for k in range(3):
            Image.new(mode, (8, 8)).save(mixed / "train" / clip / ("%d.png" % k))
    with pytest.raises(SystemExit, match="has mode L, the pool holds 3-channel frames"):
        datasets.build_pool(datasets.open_index("frames", str(mixed), True), 8, None)
    Image.new("RGBA", (8, 8)).save(mixed / "train" / "a" / "0.png")
    with pytest.raises(SystemExit, match="only L and RGB"):
        datasets.build_pool(datasets.open_index("frames", str(mixed), True), 8, None)


def test_frames_sampler_draws_and_resumes(tree):
    train, test = datasets.open_index("frames", tree, True), datasets.open_index("frames", tree, False)
    T = 5
    a, b = datasets.make_sampler(train, T, 11), datasets.make_sampler(train, T, 11)
    assert isinstance(a, datasets.FramesSampler) and not a.ordered
    draws = [a.draw() for _ in range(200)]
    assert draws == [b.draw() for _ in range(200)] and draws != [datasets.make_sampler(train, T, 12).draw() for _ in range(200)]
    bases, lengths = train.bases, train.lengths
    clips = set()
    for first, label in draws:
        s = int(np.searchsorted(bases, first, side="right")) - 1
        assert label == -1 and lengths[s] >= T and first + T <= bases[s] + lengths[s]           # inside ONE clip, never `short`
        clips.add(s)
    assert clips == {0, 1, 2} and {f - int(bases[1]) for f, _ in draws if int(bases[1]) <= f < int(bases[2])} == set(range(8))
    # the stream is the documented one: clip = randint(n) until long enough, then start = randint(0, len - T + 1)
    rng, want = np.random.RandomState(11), []
    for _ in range(20):
        while True:
            s = rng.randint(4)
            if lengths[s] >= T:
                break
        want.append(int(bases[s]) + rng.randint(0, int(lengths[s]) - T + 1))
    assert [d[0] for d in draws[:20]] == want
    pos = a.position()
    nxt = [a.draw() for _ in range(10)]
    c = datasets.make_sampler(train, T, 99)
    c.restore(pos)
    assert [c.draw() for _ in range(10)] == nxt
    # test split: the ordered walk over the clips that are long enough, from frame 0, wrapping
    walk = datasets.make_sampler(test, T, 3)
    assert walk.ordered and [walk.draw()[0] for _ in range(5)] == [0, 5, 0, 5, 0]
    pos = walk.position()
    twin = datasets.make_sampler(test, T, 4)
    twin.restore(pos)
    assert twin.draw() == walk.draw() == (5, -1)
    six = datasets.FramesSampler(types.SimpleNamespace(split="test", dataset="frames", bases=train.bases, lengths=train.lengths), 7, 0)
    assert [six.draw()[0] for _ in range(3)] == [6, 18, 6]                                       # `a` (6 frames) and `short` are skipped
    with pytest.raises(SystemExit, match="no frames test clip has 6 frames"):
        datasets.make_sampler(test, 6, 0)
    with pytest.raises(SystemExit, match="saved for BairSampler, this run draws from FramesSampler"):
        walk.restore({"sampler": "BairSampler"})
    with pytest.raises(SystemExit, match="another frames split"):
        a.restore(walk.position())


# ---- the options and the host pool ------------------------------------------------------------------------------------------------
def test_resize_options(capsys):
    import generate_frames
    import train
    for parser in (train.build_parser(), generate_frames.build_parser()):
        o = parser.parse_args([])
        assert datasets.resize_spec(o) is None and not hasattr(o, "resize")      # the default: none / crop, and the options object of before
        assert datasets.resize_spec(parser.parse_args(["--resize", "box"])) == ("box", "crop")
        assert datasets.resize_spec(parser.parse_args(["--resize", "none", "--resize_fit", "stretch"])) is None
        o = parser.parse_args(["--resize", "lanczos", "--resize_fit", "stretch"])
        assert datasets.resize_spec(o) == ("lanczos", "stretch")
        for bad in (["--resize", "nearest"], ["--resize_fit", "pad"]):
            with pytest.raises(SystemExit) as e:
                parser.parse_args(bad)
            assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    assert datasets.resize_spec(types.SimpleNamespace()) is None                      # an options object older than the flag
    for extra, named in ((["--dataset", "smmnist"], "--dataset smmnist"), (["--dataset", "frames", "--synthetic_data"], "--synthetic_data")):
        with pytest.raises(SystemExit) as e:
            train.main(extra + ["--resize", "bilinear"])
        assert str(e.value).startswith("train.py --resize:") and named in str(e.value) and "\n" not in str(e.value)
    # not part of the --resume fingerprint: it changes frame bytes, not the draw streams
    from dvg_amd import train_state
    a = train.build_parser().parse_args(["--dataset", "frames"])
    b = train.build_parser().parse_args(["--dataset", "frames", "--resize", "bicubic"])
    for o in (a, b):
        o.ft, o.world = True, 1
    assert train_state.option_fingerprint(a) == train_state.option_fingerprint(b)


def test_host_pool_resizes_like_pillow_and_refuses_without_the_flag(tree):
    index = datasets.open_index("frames", tree, True)
    with pytest.raises(SystemExit, match=r"frame0\.png' is 40x30, not 64x64"):
        datasets.build_pool(index, 64, None)
    for f, fit in (("bilinear", "crop"), ("lanczos", "stretch")):
        pool = datasets.build_pool(index, 64, None, resize=(f, fit))
        assert pool.dtype == torch.uint8 and tuple(pool.shape) == (27, 64, 64, 3)
        assert np.array_equal(pool.numpy(), frames_tree.pillow_pool(index, 64, f, fit))
    # frames that already have the size are what they were; the pool is shared per resize spec
    same = datasets.build_pool(index, 48, None, resize=("bicubic", "crop")).numpy()
    with Image.open(index.sequences[2][3]) as im:
        assert np.array_equal(same[int(index.bases[2]) + 3], np.asarray(im))
    p1 = datasets.shared_pool(index, tree, 32, None, 2, ("box", "crop"))
    assert datasets.shared_pool(index, tree, 32, None, 2, ("box", "crop")) is p1
    assert datasets.shared_pool(index, tree, 32, None, 2, ("box", "stretch")) is not p1


# ---- dvg_resample_u8: the checks before the launch ----------------------------------------------------------------------------------
def test_resample_entry_point_rejects_bad_calls_without_gpu():
    from dvg_amd import _lib, ops
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    ymin, _ = resample.tables(120, 0, 120, 64, "bilinear")
    ok = dict(src=one, dst=one, n=2, Hin=120, Win=160, Hout=64, Wout=64, C=3, xmin=one, xcoef=one, xk=7, ymin=one, ycoef=one, yk=5,
              ymin_host=ymin.ctypes.data)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dvg_resample_u8(*[a[k] for k in ok], None)
    SHAPE, NULL = 1, 2
    for ptr in ("src", "dst", "xmin", "xcoef", "ymin", "ycoef", "ymin_host"):
        assert call(**{ptr: None}) == NULL and b"dvg_resample_u8" in lib.dvg_last_error(), ptr
    for zero in ("n", "Hin", "Win", "Hout", "Wout"):
        assert call(**{zero: 0}) == SHAPE, zero
    assert call(C=2) == SHAPE and b"1 or 3" in lib.dvg_last_error()
    assert call(xk=-1) == SHAPE and call(xk=0) == SHAPE and b"no horizontal pass" in lib.dvg_last_error()      # 160 -> 64 needs one
    assert call(yk=0, ymin=None, ycoef=None, ymin_host=None) == SHAPE and b"no vertical pass" in lib.dvg_last_error()
    # a geometry whose one-row band does not fit the LDS budget: 5001 box taps, i.e. intermediate rows, of 64 x 3 bytes
    tall, coef = resample.tables(320000, 0, 320000, 64, "box")
    assert call(Hin=320000, yk=coef.shape[1], ymin_host=tall.ctypes.data) == SHAPE and b"do not fit 64 KB" in lib.dvg_last_error()
    assert call(Win=20000) == SHAPE                                                      # four source rows alone exceed it
    # the band chooser: whole frames where they fit, several bands for a tall input, 0 when nothing fits
    assert ops.resample_band(120, 160, 64, 64, 3) == (64, 120)
    band, span = ops.resample_band(1100, 40, 64, 64, 3, "lanczos")
    assert 1 <= band < 64 and 4 * ((40 * 3 + 8 + 15) // 16 * 16) + span * 64 * 3 <= 64 * 1024
    assert ops.resample_band(64, 64, 64, 64, 1) == (64, 64)                               # no pass: the band copies its own rows
    assert ops.resample_band(320000, 160, 64, 64, 3, "box")[0] == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_u8(torch.zeros(1, 8, 8, 1, dtype=torch.uint8), (4, 4))
