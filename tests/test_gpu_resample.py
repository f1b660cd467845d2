"""GPU: dvg_resample_u8 (ops.resample_u8) against Pillow's Image.resize, byte for byte: every filter, 1 and 3 channels, one frame
and five, the whole image and the crop box, random bytes and a 0 / 255 checkerboard, over the geometries of
tests/resample_cases.py - skipped passes, clipped taps, 95 taps, several bands per frame."""

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

from dvg_amd import mnist, ops, resample  # noqa: E402
from tests import resample_cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 5


@pytest.mark.parametrize("filter", resample.FILTERS)
@pytest.mark.parametrize("geometry", resample_cases.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_resample_u8_is_bit_equal_to_pillow(geometry, filter):
    H, W, S = geometry
    for C in (1, 3):
        for kind in resample_cases.KINDS:
            imgs = resample_cases.images(kind, N, H, W, C)
            src = torch.from_numpy(imgs).to(DEV)
            for box in resample_cases.boxes(H, W, S):
                want = resample_cases.pillow(imgs, S, filter, box)
                got = ops.resample_u8(src, (S, S), filter, box=box)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (N, S, S, C)
                assert np.array_equal(got.cpu().numpy(), want), (C, kind, box)
                one = ops.resample_u8(src[:1], (S, S), filter, box=box)                 # n = 1
                assert np.array_equal(one.cpu().numpy(), want[:1]), (C, kind, box, "n=1")
            if kind == "checker" and filter in ("bicubic", "lanczos") and (H, W) == (63, 65):
                assert want.min() == 0 and want.max() == 255                            # the overshoot was clamped, both ways


def test_the_geometries_take_the_paths_they_are_listed_for():
    assert ops.resample_band(64, 64, 64, 64, 3) == (64, 64)                             # a copy
    assert resample.pass_needed(48, 0, 48, 64) and not resample.pass_needed(64, 0, 64, 64)
    for f in resample.FILTERS:
        for C in (1, 3):
            band, _ = ops.resample_band(1100, 40, 64, 64, C, f)
            assert 1 <= band < 64, (f, C, band)                                          # several bands per frame
    assert resample.tables(1000, 0, 1000, 64, "lanczos")[1].shape[1] == 95


def test_the_mnist_case_equals_the_mnist_kernel():
    raw = resample_cases.images("random", 9, 28, 28, 1)
    src = torch.from_numpy(raw).to(DEV)
    got = ops.resample_u8(src, (32, 32), "bilinear")
    assert torch.equal(got[..., 0], ops.mnist_scale_u8(src[..., 0].contiguous(), 32))
    assert np.array_equal(got.cpu().numpy()[..., 0], mnist.resize_u8(raw[..., 0], 32))


def test_rectangular_target_unaligned_source_and_out_inside_a_pool():
    imgs = resample_cases.images("random", 3, 37, 53, 3)
    want = resample_cases.pillow(imgs, 64, "hamming", None)
    flat = torch.zeros(imgs.size + 1, dtype=torch.uint8, device=DEV)                     # a source that starts at an odd address
    flat[1:] = torch.from_numpy(imgs).to(DEV).reshape(-1)
    pool = torch.full((7, 64, 64, 3), 171, dtype=torch.uint8, device=DEV)
    out = ops.resample_u8(flat[1:].view(3, 37, 53, 3), (64, 64), "hamming", out=pool[2:5])
    assert out.data_ptr() == pool[2].data_ptr()
    host = pool.cpu().numpy()
    assert np.array_equal(host[2:5], want) and (host[:2] == 171).all() and (host[5:] == 171).all()   # the neighbours are untouched
    from PIL import Image
    rect = np.asarray(Image.fromarray(imgs[0]).resize((21, 30), resample.pil_filter("bicubic")))      # 30 rows of 21: 63-byte rows
    assert np.array_equal(ops.resample_u8(torch.from_numpy(imgs[:1]).to(DEV), (30, 21), "bicubic").cpu().numpy()[0], rect)
    for bad in (dict(out=pool[2:6]), dict(out=pool[:, :32]), dict(box=(0, 0, 54, 37)), dict(filter="nearest")):
        with pytest.raises(RuntimeError, match="resample_u8"):
            ops.resample_u8(torch.from_numpy(imgs).to(DEV), (64, 64), **dict(dict(filter="hamming"), **bad))
    with pytest.raises(RuntimeError, match="1 or 3"):
        ops.resample_u8(torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=DEV), (4, 4))


def test_bad_arguments_launch_nothing():
    from dvg_amd import _lib
    lib = _lib.lib()
    src = torch.from_numpy(resample_cases.images("random", 2, 120, 160, 3)).to(DEV)
    dst = torch.full((2, 64, 64, 3), 7, dtype=torch.uint8, device=DEV)
    tabs = [torch.from_numpy(t).to(DEV) for ax in ((160, 64), (120, 64)) for t in resample.tables(ax[0], 0, ax[0], ax[1], "bilinear")]
    ymin_host, _ = resample.tables(120, 0, 120, 64, "bilinear")
    stream = torch.cuda.current_stream().cuda_stream

    def call(s=src.data_ptr(), d=dst.data_ptr(), C=3, Hin=120, yk=None, yh=ymin_host):
        return lib.dvg_resample_u8(s, d, 2, Hin, 160, 64, 64, C, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[1].shape[1],
                                   tabs[2].data_ptr(), tabs[3].data_ptr(), tabs[3].shape[1] if yk is None else yk, yh.ctypes.data, stream)
    assert call(s=None) == 2 and b"NULL" in lib.dvg_last_error()
    assert call(d=None) == 2
    assert call(C=2) == 1 and b"1 or 3" in lib.dvg_last_error()
    tall, coef = resample.tables(320000, 0, 320000, 64, "box")
    assert call(Hin=320000, yk=coef.shape[1], yh=tall) == 1 and b"do not fit 64 KB" in lib.dvg_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7).all())                                                        # nothing was launched
    assert call() == 0
    assert np.array_equal(dst.cpu().numpy(), resample_cases.pillow(src.cpu().numpy(), 64, "bilinear", None))
    with pytest.raises(RuntimeError, match="do not fit 64 KB"):
        ops.resample_u8(torch.zeros(1, 70000, 4, 1, dtype=torch.uint8, device=DEV), (8, 8), "lanczos")
