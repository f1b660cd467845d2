"""CPU: the figure layouts, encoders and host-side checks behind the reference's GIF / PNG writers (dvg_amd/viz.py).

  * tests/viz_ref.py's restatement of utils.image_tensor and of the truncating byte conversion equals
    tests/golden/reference_viz.npz - outputs of the reference's own functions - exactly;
  * every layout table (make_gifs, plot, plot_rec), rendered cell by cell, equals the figure assembled the reference's way
    (add_border + nested image_tensor) exactly;
  * the random sample picks leave numpy's and torch's global streams where they were;
  * write_png / write_gif round trips; without Pillow nothing raises and PNGs are still written;
  * dvg_frame_mosaic's argument checks fire before any launch (no GPU here).
tests/test_gpu_viz.py holds the kernel to the same restatement, bit for bit."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

from dvg_amd import viz
from tests import viz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_viz():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_viz.npz"))


def test_restated_image_tensor_equals_the_reference(golden_viz):
    for name in viz_ref.GOLDEN_CASES:
        inputs, padding = viz_ref.golden_inputs(name)
        ours = viz_ref.image_tensor(inputs, padding).numpy()
        assert ours.shape == golden_viz[name].shape and np.array_equal(ours, golden_viz[name]), name
    assert set(golden_viz.files) == set(viz_ref.GOLDEN_CASES) | {"draw_text_empty"}


def test_truncating_conversion_equals_the_reference_draw_text_tensor(golden_viz):
    """draw_text_tensor(x, "") = uint8(x * 255) / 255. (utils.py:167-173): no font involved."""
    ref = golden_viz["draw_text_empty"]                              # (3, h, w) float32 = byte / 255.
    ours = viz_ref.to_bytes(viz_ref.golden_text_frame(), viz_ref.TRUNC)      # (h, w, 3) uint8
    assert np.array_equal((ours.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1), ref)
    assert np.array_equal(np.rint(ref * 255).astype(np.uint8).transpose(1, 2, 0), ours)
    # the border's 0.7f is a tie: 0.7f * 255 = 178.5 in fp32 - truncated 178, to nearest 179; an fma would not tie
    assert np.float32(0.7) * np.float32(255) == np.float32(178.5)
    px = torch.full((1, 1, 1), 0.7)
    assert viz_ref.to_bytes(px, viz_ref.TRUNC)[0, 0, 0] == 178 and viz_ref.to_bytes(px, viz_ref.NEAREST)[0, 0, 0] == 179


def figure_case(nc, seed=0, T=7, B=4, S=5, H=8):
    x = viz_ref.seeded(100 + seed, T, B, nc, H, H)
    post = viz_ref.seeded(200 + seed, T, B, nc, H, H)
    samples = viz_ref.seeded(300 + seed, S, T, B, nc, H, H)
    best = torch.tensor([2, 2, 0, 2][:B] + [1] * max(0, B - 4), dtype=torch.int64)       # repeats
    return x, post, samples, best


@pytest.mark.parametrize("n_past", [2, 5])
@pytest.mark.parametrize("nc", [1, 3])
def test_layout_tables_render_to_the_reference_figures(nc, n_past):
    x, post, samples, best = figure_case(nc)
    T, B, S, H = x.shape[0], x.shape[1], samples.shape[0], x.shape[-1]
    # make_gifs: every batch row, with label masks (synthetic ones: the layout does not depend on the font)
    lay = viz.make_gifs_layout(T, n_past, B, H, rows=B)
    assert (lay.cell_h, lay.cell_w, lay.oy, lay.ox, lay.pad_x, lay.Cc) == (H + 32, H + 2, 1, 1, 0, 6)
    assert lay.labels[0] == 'Ground\ntsruth' and lay.labels[5] == 'Random\nsample 3'
    picks = viz.random_picks(11, B, 3, S)
    masks = np.random.RandomState(5).rand(6, lay.cell_h, lay.cell_w) < 0.2
    for m in (None, masks):
        got = viz_ref.render_layout(lay, [x, post, samples], best, picks, m)
        assert got.shape == (B * T, H + 32, 6 * (H + 2), 3)
        for row in range(B):
            ref = viz_ref.make_gifs_reference(x, post, samples, best, picks[row], n_past, row, m)
            for t in range(T):
                assert np.array_equal(got[row * T + t], ref[t]), (row, t)
    lay.check([T * B, T * B, S * T * B], B, picks.shape)
    assert viz.make_gifs_layout(T, n_past, B, H).F == T          # the reference's early return: row 0 only
    # plot: PNG and GIF
    png_l, gif_l = viz.plot_layout(T, B, H)
    p4 = viz.random_picks(12, min(B, 10), 4, S)
    ref_png, ref_gif = viz_ref.plot_reference(x, samples, best, p4, T)
    got_png = viz_ref.render_layout(png_l, [x, None, samples], best, p4)
    assert got_png.shape[1:] == ref_png.shape and np.array_equal(got_png[0], ref_png)
    got_gif = viz_ref.render_layout(gif_l, [x, None, samples], best, p4)
    assert len(ref_gif) == T == got_gif.shape[0]
    for t in range(T):
        assert np.array_equal(got_gif[t], ref_gif[t]), t
    assert (gif_l.pad_y, gif_l.pad_x) == (0, 1)                   # image_tensor's quirk: the inner level pads by 1 regardless
    # plot_rec: every third frame of one batch row
    for index in (0, B - 1):
        rec = viz.plot_rec_layout(T, H, index=index, B=B)
        got = viz_ref.render_layout(rec, [x])
        assert np.array_equal(got[0], viz_ref.plot_rec_reference(x, index))
    assert viz.plot_rec_layout(105, 64).Cc == 35


def test_plot_layout_caps_the_rows_at_ten():
    png_l, gif_l = viz.plot_layout(3, 16, 8)
    assert png_l.R == 60 and gif_l.R == 10 and gif_l.F == 3


def test_random_picks_do_not_touch_the_global_streams():
    np.random.seed(3)
    torch.manual_seed(3)
    s_np, s_t = np.random.get_state(), torch.get_rng_state()
    a = viz.random_picks(1, 4, 3, 100)
    b = viz.random_picks(1, 4, 3, 100)
    rs = np.random.RandomState(1)
    c, d = viz.random_picks(rs, 4, 3, 100), viz.random_picks(rs, 4, 3, 100)
    assert a.dtype == np.int32 and a.shape == (4, 3) and np.array_equal(a, b) and np.array_equal(a, c)
    assert not np.array_equal(c, d) and a.min() >= 0 and a.max() < 100
    ref = np.random.RandomState(1)
    assert [int(v) for v in a[0]] == [ref.randint(100) for _ in range(3)]
    s_np2 = np.random.get_state()
    assert s_np[0] == s_np2[0] and np.array_equal(s_np[1], s_np2[1]) and s_np[2:] == s_np2[2:]
    assert torch.equal(s_t, torch.get_rng_state())


def decode_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, = struct.unpack(">I", raw[pos:pos + 4])
        tag, data = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff, tag
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0)
    ch = {2: 3, 0: 1}[ctype]
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, ch) if ch == 3 else rows[:, 1:]


def test_write_png_round_trip(tmp_path):
    img = np.random.RandomState(0).randint(0, 256, size=(13, 22, 3)).astype(np.uint8)      # row bytes 66: no multiple of 4
    viz.write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(decode_png(str(tmp_path / "a.png")), img)
    viz.write_png(str(tmp_path / "t.png"), torch.from_numpy(img))
    assert np.array_equal(decode_png(str(tmp_path / "t.png")), img)
    viz.write_png(str(tmp_path / "g.png"), img[:, :, 0])
    assert np.array_equal(decode_png(str(tmp_path / "g.png")), img[:, :, 0])
    with pytest.raises(TypeError):
        viz.write_png(str(tmp_path / "f.png"), img.astype(np.float32))
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "a.png")).convert("RGB")), img)


def test_write_gif_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(1)
    palette = rs.randint(0, 256, size=(200, 3)).astype(np.uint8)                        # <= 256 distinct colours
    frames = palette[rs.randint(0, 200, size=(5, 12, 22))]
    path = str(tmp_path / "a.gif")
    assert viz.write_gif(path, frames, duration=0.25) is True
    im = Image.open(path)
    assert im.n_frames == 5 and im.size == (22, 12)
    for f in range(5):
        im.seek(f)
        assert im.info["duration"] == 250
        assert np.array_equal(np.asarray(im.convert("RGB")), frames[f]), f
    # more than 256 colours: still written (quantised), same geometry
    wide = rs.randint(0, 256, size=(2, 40, 40, 3)).astype(np.uint8)
    assert viz.write_gif(str(tmp_path / "w.gif"), torch.from_numpy(wide), duration=0.1)
    im = Image.open(str(tmp_path / "w.gif"))
    assert im.n_frames == 2 and im.size == (40, 40)


def test_without_pillow_gifs_and_labels_are_skipped_with_one_warning(tmp_path, monkeypatch, capsys):
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)
    monkeypatch.setattr(viz, "_warned", set())
    frames = np.zeros((2, 4, 4, 3), dtype=np.uint8)
    assert viz.write_gif(str(tmp_path / "a.gif"), frames) is False and not os.path.exists(str(tmp_path / "a.gif"))
    x, post, samples, best = figure_case(1)
    lay = viz.make_gifs_layout(x.shape[0], 2, x.shape[1], 8)
    assert viz.render_labels(lay.labels, lay.cell_h, lay.cell_w) is None
    cells, masks = lay.upload("cpu")
    assert masks is None and cells.dtype == torch.int32 and cells.numel() == lay.F * 6 * 8
    picks = viz.random_picks(1, 1, 3, samples.shape[0])
    mosaic = viz_ref.render_layout(lay, [x, post, samples], best, picks, None)
    viz.write_png(str(tmp_path / "a.png"), mosaic[0])                      # the labelled figure still gives its PNG
    assert np.array_equal(decode_png(str(tmp_path / "a.png")), mosaic[0])
    err = capsys.readouterr().err
    assert err.count("Pillow is not installed") == 1, err


def test_label_masks_follow_the_default_font():
    pytest.importorskip("PIL.Image")
    lay = viz.make_gifs_layout(3, 2, 2, 64)
    m = viz.render_labels(lay.labels, lay.cell_h, lay.cell_w)
    assert m.shape == (6, 96, 66) and m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
    for i in range(6):
        ys, xs = np.nonzero(m[i])
        assert ys.min() >= 64 and xs.min() >= 4, i               # draw.text((4, 64), ...): below the 64-row image
    assert not np.array_equal(m[3], m[4])


def test_layout_check_rejects_out_of_range_tables():
    lay = viz.make_gifs_layout(4, 2, 3, 8, rows=3)
    lay.check([12, 12, 5 * 12], 3, (3, 3))
    with pytest.raises(ValueError):
        lay.check([11, 12, 60], 3, (3, 3))                       # ground truth one image short
    with pytest.raises(ValueError):
        lay.check([12, 12, 60], 0, (3, 3))                       # no best
    with pytest.raises(ValueError):
        lay.check([12, 12, 60], 3, (3, 2))                       # picks too narrow
    with pytest.raises(ValueError):
        lay.check([12, 12, 11], 3, (3, 3))                       # not one whole sample


def test_frame_mosaic_host_side_checks_without_gpu():
    """In the style of test_abi.py::test_host_side_checks_reject_bad_shapes_without_gpu: fake pointers, never dereferenced."""
    from dvg_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)

    def call(src0=one, n0=4, nc=1, H=8, W=8, cells=one, F=1, R=1, Cc=2, cell_h=8, cell_w=8, pad_y=0, pad_x=1, oy=0, ox=0,
             best=None, n_best=0, picks=None, rows=0, k=0, labels=None, nl=0, lh=0, lw=0, quant=0, out=one):
        return lib.dvg_frame_mosaic(src0, n0, None, 0, None, 0, nc, H, W, cells, F, R, Cc, cell_h, cell_w, pad_y, pad_x, oy,
                                    ox, best, n_best, picks, rows, k, labels, nl, lh, lw, quant, out, None)
    NULL, SHAPE = 2, 1
    assert call(cells=None) == NULL and call(out=None) == NULL and call(src0=None, n0=0) == NULL
    assert call(n0=0) == SHAPE                                   # a source without images
    assert call(nc=2) == SHAPE and call(H=0) == SHAPE and call(F=0) == SHAPE and call(pad_x=-1) == SHAPE
    assert call(oy=1) == SHAPE and b"does not fit" in lib.dvg_last_error()
    assert call(cell_w=7) == SHAPE
    assert call(quant=2) == SHAPE
    assert call(best=one, n_best=0) == SHAPE and call(n_best=3) == SHAPE
    assert call(picks=one, rows=2, k=0) == SHAPE and call(rows=2, k=3) == SHAPE
    assert call(labels=one, nl=1, lh=9, lw=8) == SHAPE and call(nl=1, lh=8, lw=8) == SHAPE
    assert call(F=40000, R=10, Cc=10, cell_h=64, cell_w=64) == SHAPE and b"32-bit" in lib.dvg_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(SHAPE, "dvg_frame_mosaic")
    from dvg_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_mosaic([torch.zeros(2, 1, 8, 8)], torch.zeros(16, dtype=torch.int32), nc=1, H=8, W=8, F=1, R=1, Cc=2,
                         cell_h=8, cell_w=8)
