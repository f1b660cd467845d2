"""CPU restatement (torch, fp32) of the reference's figure code, for tests/test_viz_host.py and tests/test_gpu_viz.py:
utils.image_tensor (utils.py:104-150), add_border (generate_frames.py:306-319), the two byte conversions, the three figure
assemblies (generate_frames.py:185-217 and :235-245, train.py:291-335) as the reference builds them - nested lists through
image_tensor - and, independently, a renderer of dvg_amd.viz layout tables.  tests/golden/reference_viz.npz (written by
tests/golden/make_golden_viz.py from the reference's own utils.py) pins image_tensor and the truncating conversion."""
import numpy as np
import torch

TRUNC, NEAREST = 0, 1


# ---- seeded inputs shared with tests/golden/make_golden_viz.py (the .npz holds outputs only) -------------------------------
def seeded(seed, *shape, lo=-0.25, hi=1.25):
    """fp32 tensor with values below 0, above 1, exactly 0.7f, 0, 1 and k/255 ties (k/255 * 255 lands on or beside an integer)."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(lo, hi, size=shape).astype(np.float32)
    flat = a.reshape(-1)
    n = flat.size
    flat[rs.permutation(n)[:max(1, n // 4)]] = (rs.randint(0, 256, size=max(1, n // 4)) / 255.0).astype(np.float32)
    special = np.array([0.7, 0.0, 1.0, 0.5, 127.5 / 255, 0.1, 0.3], dtype=np.float32)
    pos = rs.permutation(n)[:min(n, len(special))]
    flat[pos] = special[:len(pos)]
    return torch.from_numpy(a)


GOLDEN_CASES = {
    # name: (image shape, rows (None = flat list), columns, padding)
    "flat_nc1_p0": ((1, 8, 8), None, 3, 0), "flat_nc1_p1": ((1, 8, 8), None, 3, 1),
    "flat_nc3_p0": ((3, 8, 8), None, 4, 0), "flat_nc3_p1": ((3, 8, 8), None, 4, 1),
    "nested_nc1_p0": ((1, 8, 8), 3, 2, 0), "nested_nc1_p1": ((1, 8, 8), 3, 2, 1),
    "nested_nc3_p0": ((3, 8, 8), 2, 3, 0), "nested_nc3_p1": ((3, 8, 8), 2, 3, 1),
    "flat_3d_nonsquare_p1": ((1, 8, 12), None, 3, 1), "nested_3d_nonsquare_p0": ((3, 12, 8), 2, 2, 0),
    "flat_2d_nonsquare_p1": ((8, 12), None, 3, 1), "nested_2d_nonsquare_p1": ((12, 8), 2, 3, 1),
}


def golden_inputs(name):
    shape, rows, cols, padding = GOLDEN_CASES[name]
    seed = 7000 + sorted(GOLDEN_CASES).index(name) * 100
    if rows is None:
        return [seeded(seed + c, *shape) for c in range(cols)], padding
    return [[seeded(seed + r * 10 + c, *shape) for c in range(cols)] for r in range(rows)], padding


def golden_text_frame():
    """The bordered frame whose draw_text_tensor(x, "") output pins the truncating conversion (values inside [0, 1])."""
    return add_border(seeded(7999, 1, 16, 16, lo=0.0, hi=1.0).clamp(0, 1), 'red')


# ---- utils.image_tensor -----------------------------------------------------------------------------------------------------
def _nested(inputs):
    first = inputs[0]
    return isinstance(first, (list, tuple)) or (torch.is_tensor(inputs) and inputs.dim() > 4)


def image_tensor(inputs, padding=1):
    """A flat list: the images side by side on a canvas of ones, `padding` columns apart.  A list of lists: every inner list
    as a flat row WITH THE DEFAULT PADDING 1 (the recursive call passes none), the rows stacked `padding` rows apart.  2-D
    images count as one channel."""
    if _nested(inputs):
        parts = [image_tensor(row) for row in inputs]
        c, h, w = parts[0].shape
        n = len(parts)
        canvas = torch.ones(c, h * n + padding * (n - 1), w)
        for i, part in enumerate(parts):
            canvas[:, i * (h + padding):i * (h + padding) + h, :] = part
        return canvas
    imgs = list(inputs)
    c, (h, w) = (imgs[0].shape[0] if imgs[0].dim() == 3 else 1), imgs[0].shape[-2:]
    n = len(imgs)
    canvas = torch.ones(c, h, w * n + padding * (n - 1))
    for i, im in enumerate(imgs):
        canvas[:, :, i * (w + padding):i * (w + padding) + w] = im
    return canvas


def add_border(x, color, pad=1):
    """A 3 x (w+2pad+30) x (w+2pad) cell, w = x.size(1): black, or 0.7 in channel 0 (red) / 1 (green); the image at (pad, pad),
    one channel replicated to three."""
    w = x.shape[1]
    px = torch.zeros(3, w + 2 * pad + 30, w + 2 * pad)
    if color == 'red':
        px[0] = 0.7
    elif color == 'green':
        px[1] = 0.7
    px[:, pad:pad + w, pad:pad + w] = x          # (1,w,w) broadcasts over the three channels, (3,w,w) copies
    return px


def to_bytes(img, mode):
    """(C,H,W) float -> uint8 (H,W,3).  TRUNC: np.uint8(x * 255) of draw_text_tensor (utils.py:169) after the clamp of
    save_gif_with_text (:189); NEAREST: bytescale with cmin 0, cmax 1 - (x * 255).clip(0, 255) + 0.5, truncated.  Every step
    one fp32 rounding."""
    v = img.float().clamp(0, 1) * 255
    if mode == NEAREST:
        v = v + 0.5
    b = v.to(torch.uint8)
    if b.shape[0] == 1:
        b = b.expand(3, -1, -1)
    return b.permute(1, 2, 0).contiguous().numpy()


def draw_label(cell_bytes, mask):
    """draw_text_tensor's fill (0,0,0) where the (h,w) mask (anchored at the cell's corner) is set."""
    if mask is not None:
        out = cell_bytes.copy()
        h, w = mask.shape
        out[:h, :w][mask.astype(bool)] = 0
        return out
    return cell_bytes


# ---- the figures, the reference's way -----------------------------------------------------------------------------------------
def make_gifs_reference(x, posterior, samples, best, rand_sidx, n_past, row, masks=None):
    """generate_frames.py:185-217 for batch row `row`: list over t of uint8 (H+32, 6(W+2), 3).  x / posterior: (T,B,C,H,W),
    samples (S,T,B,C,H,W); labels are drawn on every bordered cell's bytes (draw_text_tensor), the six cells then joined
    with padding 0."""
    frames = []
    for t in range(x.shape[0]):
        colour = 'green' if t < n_past else 'red'
        cells = [add_border(x[t][row], 'green'), add_border(posterior[t][row], colour),
                 add_border(samples[int(best[row])][t][row], colour)]
        cells += [add_border(samples[int(s)][t][row], colour) for s in rand_sidx]
        drawn = [draw_label(to_bytes(c, TRUNC), None if masks is None else masks[i]) for i, c in enumerate(cells)]
        # image_tensor(flat list, padding=0) of the drawn cells: side by side, no canvas pixel left
        frames.append(np.concatenate(drawn, axis=1))
    return frames


def plot_reference(x, gen, best, s_rand, n_eval):
    """train.py:291-335: (png uint8 (GH,GW,3), gif frames list of uint8).  x (T,B,C,H,W), gen (S,T,B,C,H,W); s_rand[i] = the
    four random sample indices of batch row i."""
    B = x.shape[1]
    nrow = min(B, 10)
    to_plot, gifs = [], [[] for _ in range(n_eval)]
    for i in range(nrow):
        to_plot.append([x[t][i] for t in range(n_eval)])
        s_list = [int(best[i])] + [int(s) for s in s_rand[i]]
        for s in s_list:
            to_plot.append([gen[s][t][i] for t in range(n_eval)])
        for t in range(n_eval):
            gifs[t].append([x[t][i]] + [gen[s][t][i] for s in s_list])
    png = to_bytes(image_tensor(to_plot, 1), NEAREST)
    return png, [to_bytes(image_tensor(g, padding=0), TRUNC) for g in gifs]


def plot_rec_reference(frames, index):
    """generate_frames.py:235-245: frames (T,B,C,H,W) -> uint8 PNG of every third frame of batch row `index`."""
    row = [frames[t][index] for t in range(0, frames.shape[0], 3)]
    return to_bytes(image_tensor([row], 1), NEAREST)


# ---- a layout table rendered on the CPU ----------------------------------------------------------------------------------------
def render_layout(layout, sources, best=None, picks=None, masks=None):
    """uint8 (F, GH, GW, 3) of a dvg_amd.viz.Layout: what dvg_frame_mosaic computes, cell by cell."""
    nc = next(s for s in sources if s is not None).shape[-3]
    flat = [None if s is None else s.detach().cpu().float().reshape(-1, nc, layout.H, layout.W) for s in sources]
    out = np.full((layout.F, layout.grid_h, layout.grid_w, 3), 255, dtype=np.uint8)
    bg = to_bytes(torch.full((1, 1, 1), 0.7), layout.quant)[0, 0, 0]
    for f in range(layout.F):
        for r in range(layout.R):
            for c in range(layout.Cc):
                src, base, stride, sel, b, k, colour, label = (int(v) for v in layout.table[f, r, c])
                cell = np.zeros((layout.cell_h, layout.cell_w, 3), dtype=np.uint8)
                if colour in (1, 2):
                    cell[:, :, colour - 1] = bg
                s = 0 if sel == 0 else int(best[b]) if sel == 1 else int(picks[b][k])
                img = flat[src][base + s * stride]
                cell[layout.oy:layout.oy + layout.H, layout.ox:layout.ox + layout.W] = to_bytes(img, layout.quant)
                if masks is not None and label >= 0:
                    cell = draw_label(cell, np.asarray(masks[label]))
                y0, x0 = r * (layout.cell_h + layout.pad_y), c * (layout.cell_w + layout.pad_x)
                out[f, y0:y0 + layout.cell_h, x0:x0 + layout.cell_w] = cell
    return out
