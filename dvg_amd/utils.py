"""Host-side helpers of the path that the reference keeps in utils.py (restated, not imported:
the reference's utils.py needs skimage / removed scipy APIs)."""
from __future__ import annotations

import torch


def init_weights(m):
    """utils.py:304-311: Conv*/Linear ~ N(0, 0.02), bias 0; BatchNorm weight ~ N(1, 0.02), bias 0.
    Keys off class-name substrings exactly like the reference (so wrappers such as `vgg_layer` do
    not match and nn.LSTMCell keeps its default init)."""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1 or classname.find("Linear") != -1:
        m.weight.data.normal_(0.0, 0.02)
        m.bias.data.fill_(0)
    elif classname.find("BatchNorm") != -1:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)


def normalize_data(opt, dtype, sequence):
    """utils.py:86-95: (B,T,H,W,C) -> list of T tensors (B,C,H,W) on the device.
    Accepts both `x` and `(x, targets)` batches (the reference unpacks a pair, which only KTH/UCF
    provide — SURVEY.md §5 quirks); returns (list, targets-or-None)."""
    targets = None
    if isinstance(sequence, (tuple, list)):
        sequence, targets = sequence
    to_gpu = dtype is None or getattr(dtype, "is_cuda", False)
    if to_gpu and torch.is_tensor(sequence) and sequence.dtype == torch.float32:
        # One host-to-device copy of the batch as it is, the three transposes as ONE device pass: the frames are the T
        # contiguous slices of a (T,B,C,H,W) buffer.  Same values as the host-side form below (pure data movement), which
        # spent 21 ms on the host per (16,12,64,64,3) batch in strided copies and 12 pageable uploads.
        seq = sequence.cuda(non_blocking=True).transpose(0, 1).transpose(3, 4).transpose(2, 3).contiguous()
        frames = [seq[t] for t in range(seq.shape[0])]
    else:
        device = torch.device("cuda") if dtype is None else None
        seq = sequence.transpose(0, 1).transpose(3, 4).transpose(2, 3)  # (T,B,C,H,W)
        if device is not None:
            frames = [seq[t].contiguous().to(device=device, dtype=torch.float32) for t in range(seq.shape[0])]
        else:
            frames = [seq[t].contiguous().type(dtype) for t in range(seq.shape[0])]
    if targets is not None and torch.is_tensor(targets) and torch.cuda.is_available():
        targets = targets.cuda()
    return frames, targets


# ---- the image writers (utils.py:104-199) ------------------------------------------------------------------------------------
# Same signatures, same nested lists of (device) tensors as the reference passes; but nothing is gridded on the host: the
# helpers that build pixels there (add_border, draw_text_tensor, image_tensor) return DESCRIPTIONS here, and a writer turns its
# description into one cell table, one `ops.frame_mosaic` launch (dvg_frame_mosaic: selection, borders, labels, clamp and
# byte conversion on the device) and one encoder call.  Only uint8 pixels cross to the host.
class Figure:
    """What image_tensor returns here: the grid it describes, composed on demand."""

    def __init__(self, rows, pad_y, pad_x):
        self.rows, self.pad_y, self.pad_x = rows, pad_y, pad_x

    def bytes(self, quant):
        """uint8 (GH, GW, 3) device tensor."""
        return _compose_figures([self], quant)[0]


def _compose_figures(figures, quant):
    from . import viz
    pads = {(f.pad_y, f.pad_x) for f in figures}
    assert len(pads) == 1, "frames of one GIF share their padding"
    (pad_y, pad_x), = pads
    layout, source = viz.grid_layout([f.rows for f in figures], pad_y, pad_x, quant)
    return viz.compose(layout, [source])


def image_tensor(inputs, padding=1):
    """utils.py:104-150: a flat list of images side by side, a list of lists as a grid (inner level always padded by 1)."""
    from . import viz
    assert len(inputs) > 0
    return Figure(*viz.figure_grid(inputs, padding))


def add_border(x, color, pad=1):
    """generate_frames.py:306-319: a (w+2pad+30) x (w+2pad) cell of `color` ('red' / 'green' = 0.7 in that channel, else black)
    with the image at (pad, pad)."""
    from . import viz
    return viz.Cell(x, color, pad, 30)


def draw_text_tensor(tensor, text):
    """utils.py:167-173: `text` in black at (4, 64) of the cell, Pillow's default font."""
    from . import viz
    c = tensor if isinstance(tensor, viz.Cell) else viz.Cell(tensor)
    return viz.Cell(c.x, c.color, c.pad, c.extra, text)


def save_tensors_image(filename, inputs, padding=1):
    """utils.py:197-199 (-> make_image -> scipy.misc.toimage): PNG, rounded to nearest."""
    from . import viz
    viz.write_png(filename, image_tensor(inputs, padding).bytes(viz.QUANT_NEAREST))


def save_gif(filename, inputs, duration=0.25):
    """utils.py:175-182: one frame per element of `inputs`, each image_tensor(element, padding=0)."""
    from . import viz
    viz.write_gif(filename, _compose_figures([image_tensor(t, padding=0) for t in inputs], viz.QUANT_TRUNC), duration)


def save_gif_with_text(filename, inputs, text, duration=0.25):
    """utils.py:184-191: per frame a flat list of cells, each with its label, joined with padding 0."""
    from . import viz
    figs = [image_tensor([draw_text_tensor(ti, texti) for ti, texti in zip(tensor, txt)], padding=0)
            for tensor, txt in zip(inputs, text)]
    viz.write_gif(filename, _compose_figures(figs, viz.QUANT_TRUNC), duration)


# ---- evaluation metrics ------------------------------------------------------------------------------------------------------
def finn_eval_seq(gt, pred):
    """utils.py:236-256: (mse, ssim, psnr), each a (bs, T) numpy array, of T predicted frames (bs,C,H,W) against the ground
    truth - the SSIM / PSNR variant of Finn et al. (2016) and Babaeizadeh et al. (2017).  `gt` / `pred`: sequences of T device
    tensors (or stacked (T,bs,C,H,W) tensors); computed by ONE launch of dvg_eval_frames_finn, then copied to the host."""
    from . import ops
    g = gt if torch.is_tensor(gt) else torch.stack(list(gt))
    p = pred if torch.is_tensor(pred) else torch.stack(list(pred))
    ssim, psnr, mse = ops.eval_frames_finn(g, p)
    return tuple(v.t().double().cpu().numpy() for v in (mse, ssim, psnr))


def sample_diversity(samples, n_past):
    """How different the samples of make_gifs are from each other, per batch row and predicted step.  samples: the
    (S,T,B,C,H,W) device tensor of make_gifs; the steps n_past ... T - 1 are scored (ops.pairwise_frame_mse, on the device;
    every reduction of its fp32 matrix in fp64).  The reference has no counterpart: it compares samples with the ground truth only.
      pair_mse    (B, T_pred) float64: the mean of the S (S - 1) / 2 pairwise MSEs (0 for S = 1)
      pair_psnr   (B, T_pred) float64: 10 log10(1 / pair_mse), +inf where pair_mse is 0
      distinct    (B, T_pred) int64: samples s with D[s, j] > 0 for every j < s = different frames among the samples (a sample
                  holding a NaN compares > 0 with nothing and is not counted)
      matrix_last (B, S, S) float32: the last predicted step's matrix"""
    from . import ops
    m = ops.pairwise_frame_mse(samples, n_past, samples.shape[1])            # (T_pred, B, S, S)
    s = m.shape[-1]
    pair_mse = (m.double().sum((-1, -2)) / max(s * (s - 1), 1)).t()         # symmetric, zero diagonal: every pair twice
    pair_psnr = 10.0 * torch.log10(1.0 / pair_mse)
    first = (m > 0) | torch.ones(s, s, dtype=torch.bool, device=m.device).triu()   # [s, j]: j >= s, or s differs from j
    distinct = first.all(-1).sum(-1).t()
    return {"pair_mse": pair_mse.contiguous(), "pair_psnr": pair_psnr.contiguous(), "distinct": distinct.contiguous(),
            "matrix_last": m[-1]}
