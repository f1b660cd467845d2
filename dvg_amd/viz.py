"""The reference's figures: layout tables for `ops.frame_mosaic` (dvg_frame_mosaic composes the uint8 mosaic on the device),
label masks, and the PNG / GIF encoders.

Three figures (restated from the reference, not imported - its scripts execute on import):
  * make_gifs (generate_frames.py:185-217): per batch row a GIF of n_eval frames, six labelled, colour-bordered columns;
  * plot (train.py:291-335): a PNG of six sequences per batch row and a GIF of the same six side by side;
  * plot_rec (generate_frames.py:235-245): one PNG row of every third frame.
A layout is pure host data (an int32 table [F][R][Cc][8], see include/dvg_hip.h); WHICH sample a cell shows may be left to
the device (`best[b]`, `picks[b][k]`), so a table depends on shapes only.  The random sample indices come from a private
numpy RandomState: no global random stream is advanced, every tensor the entry points save stays what it was.

write_png needs the standard library only.  write_gif and the label masks need Pillow; without it they print one warning and
are skipped - PNGs are still written and nothing raises."""
from __future__ import annotations

import struct
import sys
import zlib

import numpy as np

from ._lib import CONSTANTS

QUANT_TRUNC, QUANT_NEAREST = CONSTANTS["QUANT_TRUNC"], CONSTANTS["QUANT_NEAREST"]
BLACK, RED, GREEN = (CONSTANTS["MOSAIC_" + k] for k in ("BLACK", "RED", "GREEN"))
SEL_NONE, SEL_BEST, SEL_PICK = (CONSTANTS["MOSAIC_SEL_" + k] for k in ("NONE", "BEST", "PICK"))
SRC_GT, SRC_POSTERIOR, SRC_SAMPLES = 0, 1, 2            # the header numbers the sources in prose only
CELL_INTS = CONSTANTS["MOSAIC_CELL_INTS"]
_COLOURS = {None: BLACK, 'black': BLACK, 'red': RED, 'green': GREEN}
# generate_frames.py:194-213, spelling included
MAKE_GIFS_LABELS = ('Ground\ntsruth', 'Approx.\nposterior', 'Best SSIM', 'Random\nsample 1', 'Random\nsample 2',
                    'Random\nsample 3')


class Layout:
    """One figure: F frames of an R x Cc grid of cell_h x cell_w cells, pad_y / pad_x pixels of white between them, an H x W
    image at (oy, ox) of every cell.  table[f, r, c] = (src, base, stride, sel, b, k, colour, label)."""

    def __init__(self, table, H, W, cell_h, cell_w, pad_y, pad_x, oy, ox, quant, labels=()):
        self.table = np.ascontiguousarray(table, dtype=np.int32)
        assert self.table.ndim == 4 and self.table.shape[3] == CELL_INTS
        self.F, self.R, self.Cc = self.table.shape[:3]
        self.H, self.W, self.cell_h, self.cell_w = H, W, cell_h, cell_w
        self.pad_y, self.pad_x, self.oy, self.ox, self.quant = pad_y, pad_x, oy, ox, quant
        self.labels = tuple(labels)
        self._dev = {}

    @property
    def grid_h(self):
        return self.R * self.cell_h + (self.R - 1) * self.pad_y

    @property
    def grid_w(self):
        return self.Cc * self.cell_w + (self.Cc - 1) * self.pad_x

    def check(self, counts, n_best=0, picks_shape=(0, 0)):
        """Host-side bounds of the table against the sources' image counts (the kernel checks again, per cell)."""
        t = self.table.reshape(-1, CELL_INTS).astype(np.int64)
        src, base, stride, sel, b, k = (t[:, i] for i in range(6))
        if ((src < 0) | (src > 2)).any() or ((sel < 0) | (sel > 2)).any() or (base < 0).any():
            raise ValueError("mosaic layout: source / selector / base out of range")
        cnt = np.asarray(list(counts) + [0] * (3 - len(counts)), dtype=np.int64)[src]
        plain = sel == SEL_NONE
        if (base[plain] >= cnt[plain]).any():
            raise ValueError("mosaic layout: an image index lies outside its source")
        if ((stride[~plain] <= 0) | (base[~plain] >= stride[~plain]) | (stride[~plain] > cnt[~plain])).any():
            raise ValueError("mosaic layout: a selected cell needs 0 <= base < stride <= the source's image count")
        if (b[sel == SEL_BEST] >= n_best).any() or (b[~plain] < 0).any():
            raise ValueError("mosaic layout: best[b] out of range")
        pk = sel == SEL_PICK
        if (b[pk] >= picks_shape[0]).any() or (k[pk] < 0).any() or (k[pk] >= picks_shape[1]).any():
            raise ValueError("mosaic layout: picks[b][k] out of range")
        if (t[:, 7] >= len(self.labels)).any():
            raise ValueError("mosaic layout: label out of range")

    def upload(self, device, with_labels=True):
        """(cells, label masks or None) on `device`, uploaded once per layout and device."""
        import torch
        key = (str(device), bool(with_labels))
        if key not in self._dev:
            cells = torch.from_numpy(self.table.reshape(-1)).to(device)
            masks = render_labels(self.labels, self.cell_h, self.cell_w) if with_labels and self.labels else None
            self._dev[key] = (cells, None if masks is None else torch.from_numpy(masks).to(device))
        return self._dev[key]


def _entry(src, base, stride=0, sel=SEL_NONE, b=0, k=0, colour=BLACK, label=-1):
    return (src, base, stride, sel, b, k, colour, label)


def random_picks(seed, rows, k, high):
    """int32 (rows, k) of `np.random.randint(high)` draws, row by row like the reference's per-row list comprehension
    (generate_frames.py:190, train.py:312-316), from a PRIVATE stream: RandomState(seed), or the RandomState passed as `seed`
    (an entry point keeps one, seeded from opt.seed, over its batches).  numpy's and torch's global streams are not touched."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    return np.array([[rs.randint(high) for _ in range(k)] for _ in range(rows)], dtype=np.int32).reshape(rows, k)


def make_gifs_layout(n_eval, n_past, B, H, W=None, rows=1):
    """generate_frames.py:185-217.  Frame r * n_eval + t is frame t of batch row r's GIF: ground truth (green), posterior,
    best[r], picks[r][0..2] (green while t < n_past, red after), cells (W+2+30) x (W+2) with the image at (1, 1), joined with
    padding 0.  The reference returns inside its loop after batch row 0 (:217): rows = 1."""
    W = H if W is None else W
    T = n_eval
    tab = np.zeros((rows * T, 1, 6, CELL_INTS), dtype=np.int32)
    for i in range(rows):
        for t in range(T):
            colour = GREEN if t < n_past else RED
            img = t * B + i
            cells = [_entry(SRC_GT, img, colour=GREEN, label=0),
                     _entry(SRC_POSTERIOR, img, colour=colour, label=1),
                     _entry(SRC_SAMPLES, img, T * B, SEL_BEST, i, 0, colour, 2)]
            cells += [_entry(SRC_SAMPLES, img, T * B, SEL_PICK, i, s, colour, 3 + s) for s in range(3)]
            tab[i * T + t, 0] = cells
    return Layout(tab, H, W, H + 2 + 30, W + 2, 0, 0, 1, 1, QUANT_TRUNC, MAKE_GIFS_LABELS)


def plot_layout(n_eval, B, H, W=None):
    """train.py:291-335 -> (png layout, gif layout).  nrow = min(B, 10); per batch row i six sequences: ground truth,
    best[i] (smallest summed squared error), picks[i][0..3].  PNG: save_tensors_image(to_plot) = image_tensor(list of rows,
    padding 1).  GIF: save_gif -> image_tensor(gifs[t], padding=0) per frame, whose INNER level still pads by 1
    (utils.py:111 calls image_tensor(x) with the default)."""
    W = H if W is None else W
    T, nrow = n_eval, min(B, 10)

    def six(t, i):
        img = t * B + i
        return [_entry(SRC_GT, img), _entry(SRC_SAMPLES, img, T * B, SEL_BEST, i)] + \
               [_entry(SRC_SAMPLES, img, T * B, SEL_PICK, i, k) for k in range(4)]
    png = np.zeros((1, nrow * 6, T, CELL_INTS), dtype=np.int32)
    gif = np.zeros((T, nrow, 6, CELL_INTS), dtype=np.int32)
    for i in range(nrow):
        for t in range(T):
            cells = six(t, i)
            gif[t, i] = cells
            for q in range(6):
                png[0, i * 6 + q, t] = cells[q]
    return (Layout(png, H, W, H, W, 1, 1, 0, 0, QUANT_NEAREST), Layout(gif, H, W, H, W, 0, 1, 0, 0, QUANT_TRUNC))


def plot_rec_layout(n_frames, H, W=None, index=0, B=1):
    """generate_frames.py:235-245: one row (nrow = min(batch_size, 1)) of frames 0, 3, 6, ... of batch row `index` of a
    (T, B, C, H, W) source, padding 1."""
    W = H if W is None else W
    ts = list(range(0, n_frames, 3))
    tab = np.zeros((1, 1, len(ts), CELL_INTS), dtype=np.int32)
    for c, t in enumerate(ts):
        tab[0, 0, c] = _entry(SRC_GT, t * B + index)
    return Layout(tab, H, W, H, W, 1, 1, 0, 0, QUANT_NEAREST)


def compose(layout, sources, best=None, picks=None, with_labels=True):
    """The layout's mosaic, uint8 (F, GH, GW, 3) on the device of the sources.  best: int64 device tensor; picks: int32
    (rows, k), a device tensor or a host array (uploaded here)."""
    import torch
    from . import ops
    srcs = [None if s is None else s.contiguous() for s in sources]
    first = next(s for s in srcs if s is not None)
    if first.dim() < 3 or tuple(first.shape[-2:]) != (layout.H, layout.W):
        raise ValueError(f"mosaic sources must end in (C, {layout.H}, {layout.W}), got {tuple(first.shape)}")
    nc = first.shape[-3]
    if picks is not None and not torch.is_tensor(picks):
        picks = torch.from_numpy(np.ascontiguousarray(picks, dtype=np.int32)).to(first.device)
    counts = [0 if s is None else s.numel() // (nc * layout.H * layout.W) for s in srcs]
    layout.check(counts, 0 if best is None else best.shape[0], (0, 0) if picks is None else tuple(picks.shape))
    cells, masks = layout.upload(first.device, with_labels)
    return ops.frame_mosaic(srcs, cells, nc=nc, H=layout.H, W=layout.W, F=layout.F, R=layout.R, Cc=layout.Cc,
                            cell_h=layout.cell_h, cell_w=layout.cell_w, pad_y=layout.pad_y, pad_x=layout.pad_x,
                            oy=layout.oy, ox=layout.ox, best=best, picks=picks, labels=masks, quant=layout.quant)


class PlotWriter:
    """train.py:291-335 on Trainer.plot()'s result (gen (S,T,B,C,H,W), best (B,)): `<out_dir>/sample_<epoch>.png` - per batch
    row, up to ten: the ground truth, the smallest-error sample best[i] and four random samples, n_eval frames each - and
    `sample_<epoch>.gif`, the same six side by side per frame.  `best` is never read back; the random indices come from a
    stream of the writer's own, seeded from opt.seed.  Returns (png path, gif path or None without Pillow)."""

    def __init__(self, seed):
        self.rng, self.layouts = np.random.RandomState(seed), {}

    def __call__(self, x, gen, best, epoch, out_dir):
        import os
        import torch
        T, B = gen.shape[1], gen.shape[2]
        H, W = gen.shape[-2:]
        key = (T, B, H, W)
        if key not in self.layouts:
            self.layouts[key] = plot_layout(T, B, H, W)
        png_l, gif_l = self.layouts[key]
        picks = torch.from_numpy(random_picks(self.rng, min(B, 10), 4, gen.shape[0])).to(gen.device)
        sources = [torch.stack(list(x[:T])), None, gen]
        os.makedirs(out_dir, exist_ok=True)
        png, gif = '%s/sample_%d.png' % (out_dir, epoch), '%s/sample_%d.gif' % (out_dir, epoch)
        write_png(png, compose(png_l, sources, best=best, picks=picks)[0])
        ok = write_gif(gif, compose(gif_l, sources, best=best, picks=picks))
        return png, (gif if ok else None)


# ---- the reference's nested lists (utils.image_tensor and friends) as one mosaic -------------------------------------------
class Cell:
    """add_border(x, color, pad) / draw_text_tensor(x, text) deferred: an image with a `pad`-wide border of `color`, `extra`
    more rows below (add_border's 30) and a label, drawn by the mosaic kernel instead of being materialised."""

    def __init__(self, x, color=None, pad=0, extra=0, text=None):
        self.x, self.color, self.pad, self.extra, self.text = x, color, pad, extra, text


def figure_grid(inputs, padding):
    """utils.image_tensor's reading of its argument -> (rows, pad_y, pad_x): a list of lists (or a tensor of more than four
    dims) is a grid whose rows are joined with `padding` and whose INNER level always pads by 1; a flat list is one row
    joined with `padding`."""
    first = inputs[0]
    if isinstance(first, (list, tuple)) or (hasattr(inputs, "dim") and inputs.dim() > 4):
        return [list(row) for row in inputs], padding, 1
    return [list(inputs)], 0, padding


def grid_layout(frames, pad_y, pad_x, quant):
    """frames: list of grids; a grid is a list of rows; a row a list of cells (tensor (C,H,W) / (H,W) or Cell), every cell
    of the same geometry.  Returns (layout, source): the distinct tensors stacked into ONE source on their device."""
    import torch
    def as_cell(c):
        return c if isinstance(c, Cell) else Cell(c)
    c0 = as_cell(frames[0][0][0])
    H, W = c0.x.shape[-2:]
    pad, extra = c0.pad, c0.extra
    # add_border sizes the cell by x.size()[1] in both directions (generate_frames.py:307-309): the images are square there
    cell_h, cell_w = H + 2 * pad + extra, W + 2 * pad
    R, Cc = len(frames[0]), len(frames[0][0])
    tab = np.zeros((len(frames), R, Cc, CELL_INTS), dtype=np.int32)
    tensors, index, labels = [], {}, []
    for f, grid in enumerate(frames):
        assert len(grid) == R, "every frame needs the same grid"
        for r, row in enumerate(grid):
            assert len(row) == Cc, "every row needs the same number of images"
            for c, cell in enumerate(row):
                bd = as_cell(cell)
                x = bd.x
                assert tuple(x.shape[-2:]) == (H, W) and (bd.pad, bd.extra) == (pad, extra), "cells of one geometry only"
                if id(x) not in index:
                    index[id(x)] = len(tensors)
                    tensors.append(x.detach().reshape((-1, H, W)).float())
                label = -1
                if bd.text:
                    if bd.text not in labels:
                        labels.append(bd.text)
                    label = labels.index(bd.text)
                tab[f, r, c] = _entry(0, index[id(x)], colour=_COLOURS[bd.color], label=label)
    return Layout(tab, H, W, cell_h, cell_w, pad_y, pad_x, pad, pad, quant, labels), torch.stack(tensors)


# ---- label masks ----------------------------------------------------------------------------------------------------------
_warned = set()


def _pillow(what):
    """PIL, or None after one warning per process."""
    try:
        import PIL.Image
        import PIL.ImageDraw  # noqa: F401
        return PIL
    except ImportError:
        if "pillow" not in _warned:
            _warned.add("pillow")
            print(f"WARNING: Pillow is not installed: {what} skipped (GIFs and text labels need it; PNGs are still written)",
                  file=sys.stderr)
        return None


def render_labels(texts, cell_h, cell_w):
    """uint8 (len(texts), cell_h, cell_w): 1 where draw_text_tensor (utils.py:167-173) paints `draw.text((4, 64), text,
    (0,0,0))` with Pillow's default font.  None without Pillow or without any text."""
    if not texts:
        return None
    pil = _pillow("text labels")
    if pil is None:
        return None
    out = np.zeros((len(texts), cell_h, cell_w), dtype=np.uint8)
    for i, text in enumerate(texts):
        img = pil.Image.new("L", (cell_w, cell_h), 0)
        draw = pil.ImageDraw.Draw(img)
        draw.fontmode = "1"                  # no anti-aliasing: a pixel is label or it is not
        draw.text((4, 64), text, 255)
        out[i] = np.asarray(img) > 0
    return out


# ---- encoders -------------------------------------------------------------------------------------------------------------
def _to_numpy(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"expected uint8 pixels, got {a.dtype}")
    return a


def write_png(path, img):
    """8-bit PNG of a uint8 (H, W, 3) RGB or (H, W) grey image; zlib only."""
    a = np.ascontiguousarray(_to_numpy(img))
    if a.ndim == 3 and a.shape[2] == 3:
        colour_type = 2
    elif a.ndim == 2:
        colour_type = 0
    else:
        raise ValueError(f"write_png: shape {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + a[0].size), dtype=np.uint8)          # filter type 0 in front of every scanline
    rows[:, 1:] = a.reshape(h, -1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def write_gif(path, frames, duration=0.25):
    """Animated GIF of uint8 (F, H, W, 3) frames, `duration` seconds each (utils.save_gif's imageio.mimsave), through Pillow.
    A sequence of at most 256 distinct colours is stored exactly (one explicit palette); otherwise Pillow quantises every
    frame.  Returns False (after one warning) when Pillow is missing."""
    a = _to_numpy(frames)
    if a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"write_gif: shape {a.shape}")
    pil = _pillow(f"{path}")
    if pil is None:
        return False
    packed = a[..., 0].astype(np.uint32) << 16 | a[..., 1].astype(np.uint32) << 8 | a[..., 2]
    colours, inverse = np.unique(packed, return_inverse=True)
    if len(colours) <= 256:
        pal = np.zeros((256, 3), dtype=np.uint8)
        pal[:len(colours)] = np.stack([colours >> 16, colours >> 8 & 255, colours & 255], 1)
        idx = inverse.reshape(a.shape[:3]).astype(np.uint8)
        ims = []
        for f in range(a.shape[0]):
            im = pil.Image.fromarray(idx[f], "P")
            im.putpalette(pal.tobytes())
            ims.append(im)
    else:
        ims = [pil.Image.fromarray(a[f], "RGB").quantize(256) for f in range(a.shape[0])]
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], duration=int(round(duration * 1000)), loop=0,
                optimize=False)
    return True
