"""The HBM-bound ends of the backbones (edge_layers.hip, misc_kernels.hip): first conv on the raw frame, the fused first
pair, the last transposed conv as projection + gather (with the loop-invariant skip part cached), SSIM / PSNR, Moving-MNIST
compositing."""
from __future__ import annotations

import numpy as np
import torch

from .._derived import derived, register
from .._lib import CONSTANTS, check, lib
from ._core import ACT_LRELU, ACT_SIGMOID, ACT_TANH, _dev_f32, _p, _run, _stream, is_nhwc, nhwc_empty
from .conv import SharedBlocks, _stats_buf, _wp_dims


def conv3x3_first(x_nchw, w, scale, shift, *, act=ACT_LRELU, slope=0.2, stats=False):
    _dev_f32(x_nchw, "conv3x3_first.x")
    x = x_nchw if x_nchw.is_contiguous() else x_nchw.contiguous()
    n, nc, h, wd = x.shape
    w = w.detach()
    cout = w.shape[0]
    if tuple(w.shape) != (cout, nc, 3, 3) or not w.is_contiguous():
        raise RuntimeError("conv3x3_first: weight must be contiguous (Cout,nc,3,3)")
    y = nhwc_empty(n, cout, h, wd, x.device)
    st = _stats_buf(lib().dvg_conv_first_stats_rows(3, n, h, wd), cout, x.device, 1) if stats else None
    _run("conv3x3_first", 2.0 * n * h * wd * cout * 9 * nc, 4.0 * (x.numel() + n * h * wd * cout),
         lib().dvg_conv3x3_first, _p(x), _p(w), _p(scale), _p(shift), _p(y), _p(st), n, h, wd, nc, cout, act, slope,
         _stream())
    return (y, st) if stats else y


def first_pair_ok(n, nc, h, w, cout) -> bool:
    """Shapes `conv3x3_first_pair` takes: one input channel, 8 x 16 tiles, a launch that fills the chip."""
    return nc == 1 and h % 8 == 0 and w % 16 == 0 and cout % 64 == 0 and n * (h // 8) * (w // 16) * (cout // 64) >= 512


def _first_pair(wx, x_nchw, w0, scale0, shift0, w1, scale1, shift1, act, slope, pool, y_from):
    """The body of conv3x3_first_pair (wx False) and conv3x3_first_pair_wx (True).  They differ in the taps of the packed 64 ->
    Cout weight (9 / 12), the workgroup floor (the direct form's alone), the products executed per output (9 / 6 x 64; `alg` is
    the direct form's count) and the entry point."""
    name, wname = ("conv3x3_first_pair_wx", "wx1") if wx else ("conv3x3_first_pair", "wp1")
    _dev_f32(x_nchw, name + ".x")
    x = x_nchw if x_nchw.is_contiguous() else x_nchw.contiguous()
    n, nc, h, wd = x.shape
    taps, cout, cin = _wp_dims(w1)
    w0 = w0.detach()
    ok = h % 8 == 0 and wd % 16 == 0 if wx else first_pair_ok(n, nc, h, wd, cout)
    if nc != 1 or tuple(w0.shape) != (9, 64) or not w0.is_contiguous() or (taps, cin) != (12 if wx else 9, 64) or not ok:
        raise RuntimeError(f"{name}: unsupported shapes x {tuple(x.shape)} w0 {tuple(w0.shape)} {wname} {tuple(w1.shape)}")
    if not 0 <= y_from <= n or (y_from and not pool):
        raise RuntimeError(f"{name}: y_from needs the pooled output and 0 <= y_from <= N")
    y = nhwc_empty(n - y_from, cout, h, wd, x.device) if y_from < n else None
    yp = nhwc_empty(n, cout, h // 2, wd // 2, x.device) if pool else None
    alg = 2.0 * n * h * wd * (64 * 9 + cout * 9 * 64)
    flops = 2.0 * n * h * wd * (64 * 9 + cout * 6 * 64) if wx else alg
    _run("conv3x3_igemm", flops, 4.0 * (x.numel() + (0 if y is None else y.numel()) + (0 if yp is None else yp.numel()) + w1.numel()),
         lib().dvg_conv3x3_first_pair_wx if wx else lib().dvg_conv3x3_first_pair, _p(x), _p(w0), _p(scale0), _p(shift0), _p(w1),
         _p(scale1), _p(shift1), _p(y), _p(yp), n, h, wd, cout, act, slope, y_from, _stream(), alg_flops=alg)
    return (y, yp) if pool else y


def conv3x3_first_pair(x_nchw, w0, scale0, shift0, wp1, scale1, shift1, *, act=ACT_LRELU, slope=0.2, pool=False, y_from=0):
    """vgg_layer(1, 64) -> vgg_layer(64, Cout) (+ 2x2 max-pool) of the encoder's first stage in eval mode as ONE launch
    (dvg_conv3x3_first_pair): the 64-channel activation between the two layers is never materialised.
    w0: the first layer's (64,1,3,3) weight as a contiguous (9, 64) tensor [tap][channel].
    y_from (pool only): the full-resolution output is stored for the images [y_from, N) only - y has N - y_from images, None
    when y_from == N (a rollout discards the skip tensors of every frame but the last conditioning one)."""
    return _first_pair(False, x_nchw, w0, scale0, shift0, wp1, scale1, shift1, act, slope, pool, y_from)


def conv3x3_first_pair_wx(x_nchw, w0, scale0, shift0, wx1, scale1, shift1, *, act=ACT_LRELU, slope=0.2, pool=False, y_from=0):
    """conv3x3_first_pair with the 64 -> Cout layer in the WX form (dvg_conv3x3_first_pair_wx; wx1: pack_wx_weight): 12 instead
    of 18 products per output pair.  `flops` is what the launch executes, `alg_flops` the direct form's count."""
    return _first_pair(True, x_nchw, w0, scale0, shift0, wx1, scale1, shift1, act, slope, pool, y_from)


def convT3x3_last(x, w, bias, nc, *, act=ACT_SIGMOID):
    _dev_f32(x, "convT3x3_last.x")
    assert is_nhwc(x)
    n, cin, h, wd = x.shape
    w = w.detach()
    if tuple(w.shape) != (cin, nc, 3, 3) or not w.is_contiguous():
        raise RuntimeError("convT3x3_last: weight must be contiguous (Cin,nc,3,3)")
    y = torch.empty((n, nc, h, wd), device=x.device, dtype=torch.float32)
    _run("convT3x3_last", 2.0 * n * h * wd * cin * 9 * nc, 4.0 * (x.numel() + y.numel()),
         lib().dvg_convT3x3_last, _p(x), _p(w), _p(bias), _p(y), n, h, wd, cin, nc, act, _stream())
    return y


def conv4x4s2_first(x_nchw, w, scale, shift, *, act=ACT_LRELU, slope=0.2, stats=False):
    _dev_f32(x_nchw, "conv4x4s2_first.x")
    x = x_nchw if x_nchw.is_contiguous() else x_nchw.contiguous()
    n, nc, h, wd = x.shape
    w = w.detach()
    cout = w.shape[0]
    if tuple(w.shape) != (cout, nc, 4, 4) or not w.is_contiguous():
        raise RuntimeError("conv4x4s2_first: weight must be contiguous (Cout,nc,4,4)")
    y = nhwc_empty(n, cout, h // 2, wd // 2, x.device)
    st = _stats_buf(lib().dvg_conv_first_stats_rows(4, n, h, wd), cout, x.device, 1) if stats else None
    _run("conv4x4s2_first", 2.0 * n * (h // 2) * (wd // 2) * cout * 16 * nc, 4.0 * (x.numel() + y.numel()),
         lib().dvg_conv4x4s2_first, _p(x), _p(w), _p(scale), _p(shift), _p(y), _p(st), n, h, wd, nc, cout, act, slope,
         _stream())
    return (y, st) if stats else y


def convT4x4s2_last(x, skip, w, bias, nc, *, act=ACT_TANH):
    _dev_f32(x, "convT4x4s2_last.x")
    assert is_nhwc(x)
    n, c1, h, wd = x.shape
    c2 = 0
    if skip is not None:
        assert is_nhwc(skip)
        c2 = skip.shape[1]
    w = w.detach()
    if tuple(w.shape) != (c1 + c2, nc, 4, 4) or not w.is_contiguous():
        raise RuntimeError("convT4x4s2_last: weight must be contiguous (Cin,nc,4,4)")
    y = torch.empty((n, nc, 2 * h, 2 * wd), device=x.device, dtype=torch.float32)
    _run("convT4x4s2_last", 2.0 * n * h * wd * (c1 + c2) * 16 * nc,
         4.0 * (x.numel() + (skip.numel() if c2 else 0) + y.numel()), lib().dvg_convT4x4s2_last, _p(x), _p(skip),
         _p(w), _p(bias), _p(y), n, h, wd, c1, c2, nc, act, _stream())
    return y


def pixel_proj(x, wm):
    """d[px][t] = sum_c x[px][c] wm[t][c] over the pixels of an NHWC-in-memory activation (dvg_pixel_proj)."""
    assert is_nhwc(x)
    n, c, h, wd = x.shape
    t = wm.shape[0]
    d = torch.empty((n * h * wd, t), device=x.device, dtype=torch.float32)
    _run("pixel_proj", 2.0 * n * h * wd * c * t, 4.0 * (x.numel() + d.numel()), lib().dvg_pixel_proj, _p(x), _p(wm),
         _p(d), n * h * wd, c, t, _stream())
    return d


_SKIP_PROJ_CACHE = {}   # id(skip) -> (weakref(skip), skip._version, id(w), w._version, d2)


def clear_skip_proj_cache():
    """Drop cached skip projections (graphs.skip_scope calls this around a group of captures: buffers allocated while
    capturing belong to the graph's pool and must not leak into eager calls, nor the reverse)."""
    _SKIP_PROJ_CACHE.clear()


register("skip_proj", clear_skip_proj_cache, _SKIP_PROJ_CACHE.values, skip_keyed=(_SKIP_PROJ_CACHE,))


def _cached_skip_proj(skip, wm_fn, w):
    """The skip tensor of a rollout is frozen after the conditioning frames (generate_frames.py:154-157), so its
    share of the last layer's projection is computed once and reused while (tensor identity, version, weight
    version) stay the same.  Inference only (callers route training through autograd)."""
    import weakref
    key = id(skip)
    ent = _SKIP_PROJ_CACHE.get(key)
    if ent is not None and ent[0]() is skip and ent[1] == skip._version and ent[2] == id(w) and ent[3] == w._version:
        return ent[4]
    d2 = pixel_proj(skip, wm_fn())
    if len(_SKIP_PROJ_CACHE) > 8:
        _SKIP_PROJ_CACHE.clear()
    _SKIP_PROJ_CACHE[key] = (weakref.ref(skip), skip._version, id(w), w._version, d2)
    return d2


def _last_wmat(wpart, t):
    return wpart.permute(2, 3, 1, 0).reshape(t, wpart.shape[0]).contiguous()          # [(kh,kw,co)][ci]


def _last_wmat_cached(w, lo, hi, t):
    """[(kh,kw,co)][ci] projection matrix of rows lo:hi of the last layer's ConvTranspose2d weight, per weight version (it
    used to be re-permuted and copied on every decoder call)."""
    return derived(w, ("wmat", lo, hi), (w,), lambda: _last_wmat(w.detach()[lo:hi], t))


def precompute_skip_proj(skip, w, ks: int) -> None:
    """The frozen skip tensor's share of the last layer's per-pixel projection, computed ahead of the first decoder call
    (rollout.condition(), second stream); convT_last_two_step then finds it in the cache."""
    wdet = w.detach()
    c1 = wdet.shape[0] - skip.shape[1]
    t = ks * ks * wdet.shape[1]
    _cached_skip_proj(skip, lambda: _last_wmat_cached(w, c1, wdet.shape[0], t), w)


class LastProj:
    """What the conv before the last layer hands over instead of its activation when it has projected it already
    (conv.convT4x4s2_proj): d = pixel_proj(activation, wmat of `w`), (N*H*W, T); shape = the activation's (N,C,H,W)."""

    def __init__(self, d, shape, w):
        self.d, self.shape, self.w = d, tuple(shape), w


def convT_last_two_step(x, skip, w, bias, nc, ks, *, act):
    """Last layer as per-pixel projection (dvg_pixel_proj: reads the activation once) + shifted sum
    (dvg_convT_gather).  x / skip NHWC-in-memory; w the original ConvTranspose2d weight (Cin,nc,ks,ks); returns
    NCHW frames.  x may be a LastProj: the first step has been done by the launch that made the activation."""
    wdet = w.detach()
    t = ks * ks * nc
    if isinstance(x, LastProj):
        if x.w is not w or tuple(x.d.shape) != (x.shape[0] * x.shape[2] * x.shape[3], t):
            raise RuntimeError("convT_last_two_step: the projection handed over was made for another last layer")
        n, c1, h, wd = x.shape
        d1 = x.d
    else:
        assert is_nhwc(x)
        n, c1, h, wd = x.shape
        d1 = pixel_proj(x, _last_wmat_cached(w, 0, c1, t))
    d2 = None
    d2_map, d2_blk = None, 0
    if isinstance(skip, SharedBlocks):      # time-batched decoder calls: the projection of the DISTINCT skip blocks only
        d2 = pixel_proj(skip.t, _last_wmat_cached(w, c1, wdet.shape[0], t))
        d2_map, d2_blk = skip.map_dev, skip.block
        if n != skip.groups * skip.block:
            raise RuntimeError("convT_last_two_step: shared skip does not match the batch")
    elif skip is not None:
        d2 = _cached_skip_proj(skip, lambda: _last_wmat_cached(w, c1, wdet.shape[0], t), w)
    s = 2 if ks == 4 else 1
    y = torch.empty((n, nc, s * h, s * wd), device=d1.device, dtype=torch.float32)
    _run("convT_gather", 0.0, 4.0 * (d1.numel() * (2 if skip is not None else 1) + y.numel()), lib().dvg_convT_gather,
         _p(d1), _p(d2), _p(bias), _p(y), ks, n, h, wd, nc, act, _p(d2_map), d2_blk, _stream())
    return y


def eval_frames(gt, pred):
    """(ssim, psnr), each (B,), of a predicted NCHW frame batch against the ground truth: per-channel skimage-style
    metrics (dvg_eval_frames) averaged over channels as utils.eval_seq does (utils.py:227-232)."""
    _dev_f32(gt, "eval_frames.gt")
    _dev_f32(pred, "eval_frames.pred")
    if gt.shape != pred.shape or gt.dim() != 4:
        raise RuntimeError(f"eval_frames: shapes {tuple(gt.shape)} vs {tuple(pred.shape)}")
    gt = gt if gt.is_contiguous() else gt.contiguous()
    pred = pred if pred.is_contiguous() else pred.contiguous()
    b, c, h, w = gt.shape
    out = torch.empty((2, b, c), device=gt.device, dtype=torch.float32)
    _run("eval_frames", 0.0, 8.0 * gt.numel(), lib().dvg_eval_frames, _p(gt), _p(pred), _p(out[0]), _p(out[1]), b * c, h,
         w, _stream())
    return out[0].mean(1), out[1].mean(1)


def eval_frames_finn(gt, pred):
    """(ssim, psnr, mse) of predicted frames against the ground truth as utils.finn_eval_seq scores them (utils.py:236-256,
    dvg_eval_frames_finn): 11x11 Gaussian-window SSIM and 10 log10(1 / mse) PSNR per channel, averaged over channels, and the
    MSE of the whole frame.  gt / pred: NCHW -> three (N,) tensors, or (T,N,C,H,W) stacked frames -> three (T,N) tensors,
    all time steps in ONE launch."""
    _dev_f32(gt, "eval_frames_finn.gt")
    _dev_f32(pred, "eval_frames_finn.pred")
    if gt.shape != pred.shape or gt.dim() not in (4, 5):
        raise RuntimeError(f"eval_frames_finn: shapes {tuple(gt.shape)} vs {tuple(pred.shape)}")
    gt = gt if gt.is_contiguous() else gt.contiguous()
    pred = pred if pred.is_contiguous() else pred.contiguous()
    lead, (c, h, w) = tuple(gt.shape[:-3]), gt.shape[-3:]
    n = gt.numel() // (c * h * w)
    out = torch.empty((2, n, c), device=gt.device, dtype=torch.float32)
    mse = torch.empty(n, device=gt.device, dtype=torch.float32)
    _run("eval_frames_finn", 0.0, 8.0 * gt.numel(), lib().dvg_eval_frames_finn, _p(gt), _p(pred), _p(out[0]), _p(out[1]),
         _p(mse), n, c, h, w, _stream())
    if c == 1:          # the mean over one channel is that channel
        return out[0].view(lead), out[1].view(lead), mse.view(lead)
    return out[0].mean(1).view(lead), out[1].mean(1).view(lead), mse.view(lead)


def pairwise_frame_mse(samples, lo=None, hi=None):
    """(hi - lo, B, S, S) mean squared differences BETWEEN the S samples of every frame (dvg_pairwise_frame_mse): entry
    [t, b, i, j] = mean over C*H*W of (samples[i, lo + t, b] - samples[j, lo + t, b])^2, computed as differences (identical
    frames give exactly 0; symmetric bit for bit; zero diagonal).  samples: the (S,T,B,C,H,W) tensor make_gifs returns,
    contiguous; [lo, hi) a step range (default: all T).  The range is scored where it lies: the strides go to the kernel."""
    _dev_f32(samples, "pairwise_frame_mse.samples")
    if samples.dim() != 6 or samples.numel() == 0 or not samples.is_contiguous():
        raise RuntimeError(f"pairwise_frame_mse: samples {tuple(samples.shape)} must be a contiguous non-empty (S,T,B,C,H,W) tensor")
    s, t, b = samples.shape[:3]
    d = samples[0, 0, 0].numel()
    lo, hi = 0 if lo is None else int(lo), t if hi is None else int(hi)
    if not 0 <= lo < hi <= t:
        raise RuntimeError(f"pairwise_frame_mse: step range [{lo}, {hi}) of {t} steps")
    if d >= 1 << 31 or (hi - lo) * b >= 1 << 31:
        raise RuntimeError(f"pairwise_frame_mse: {hi - lo}x{b} frames of {d} floats exceed the kernel's 32-bit counts")
    out = torch.empty((hi - lo, b, s, s), device=samples.device, dtype=torch.float32)
    n = (hi - lo) * b
    _run("pairwise_frame_mse", 3.0 * n * d * (s * (s - 1) // 2), 4.0 * n * d * s + 4.0 * out.numel(),
         lib().dvg_pairwise_frame_mse, _p(samples[0, lo]), _p(out), s, t * b * d, n, d, d, _stream())
    return out


QUANT_TRUNC, QUANT_NEAREST = CONSTANTS["QUANT_TRUNC"], CONSTANTS["QUANT_NEAREST"]
MOSAIC_BLACK, MOSAIC_RED, MOSAIC_GREEN = (CONSTANTS["MOSAIC_" + k] for k in ("BLACK", "RED", "GREEN"))       # cell colours
MOSAIC_SEL_NONE, MOSAIC_SEL_BEST, MOSAIC_SEL_PICK = (CONSTANTS["MOSAIC_SEL_" + k] for k in ("NONE", "BEST", "PICK"))
MOSAIC_CELL_INTS = CONSTANTS["MOSAIC_CELL_INTS"]        # {src, base, stride, sel, b, k, colour, label}


def frame_mosaic(sources, cells, *, nc, H, W, F, R, Cc, cell_h, cell_w, pad_y=0, pad_x=0, oy=0, ox=0, best=None,
                 picks=None, labels=None, quant=QUANT_TRUNC):
    """uint8 (F, GH, GW, 3) mosaics of images picked from up to three fp32 device tensors by the DEVICE cell table `cells`
    (int32, F*R*Cc*8 entries; include/dvg_hip.h: dvg_frame_mosaic).  `sources[i]`: None or a contiguous tensor that is a
    run of nc x H x W images (any leading dims).  `best` (int64, 1-D) / `picks` (int32, 2-D) / `labels` (uint8, (n, lh, lw))
    stay on the device: nothing here reads a value back, so the call does not synchronise."""
    srcs = list(sources) + [None] * (3 - len(sources))
    if len(srcs) != 3:
        raise RuntimeError("frame_mosaic: at most three sources")
    dev, counts = None, []
    for i, s in enumerate(srcs):
        if s is None:
            counts.append(0)
            continue
        _dev_f32(s, f"frame_mosaic.sources[{i}]")
        if not s.is_contiguous() or s.numel() == 0 or s.numel() % (nc * H * W):
            raise RuntimeError(f"frame_mosaic: source {i} {tuple(s.shape)} is not a contiguous run of {nc}x{H}x{W} images")
        counts.append(s.numel() // (nc * H * W))
        dev = s.device
    if dev is None:
        raise RuntimeError("frame_mosaic: no source")

    def aux(t, dtype, dim, name):
        if t is None:
            return
        if not t.is_cuda or t.dtype != dtype or t.dim() != dim or not t.is_contiguous() or t.numel() == 0:
            raise RuntimeError(f"frame_mosaic: {name} must be a contiguous {dim}-D {dtype} device tensor")
    # a column of an argsort is a strided view: packed here (a device copy, no read-back)
    best, picks = (None if t is None else t.contiguous() for t in (best, picks))
    aux(best, torch.int64, 1, "best")
    aux(picks, torch.int32, 2, "picks")
    aux(labels, torch.uint8, 3, "labels")
    if not cells.is_cuda or cells.dtype != torch.int32 or not cells.is_contiguous() or \
            cells.numel() != F * R * Cc * MOSAIC_CELL_INTS:
        raise RuntimeError(f"frame_mosaic: cells must be a contiguous int32 device tensor of {F}x{R}x{Cc}x{MOSAIC_CELL_INTS}")
    gh, gw = R * cell_h + (R - 1) * pad_y, Cc * cell_w + (Cc - 1) * pad_x
    out = torch.empty((F, gh, gw, 3), device=dev, dtype=torch.uint8)
    read = 4.0 * nc * H * W * F * R * Cc
    _run("frame_mosaic", 0.0, read + out.numel(), lib().dvg_frame_mosaic, _p(srcs[0]), counts[0], _p(srcs[1]), counts[1],
         _p(srcs[2]), counts[2], nc, H, W, _p(cells), F, R, Cc, cell_h, cell_w, pad_y, pad_x, oy, ox, _p(best),
         0 if best is None else best.shape[0], _p(picks), 0 if picks is None else picks.shape[0],
         0 if picks is None else picks.shape[1], _p(labels), *((0, 0, 0) if labels is None else labels.shape), quant,
         _p(out), _stream())
    return out


def moving_mnist_compose(sprites, ids, pos, seq_len, image_size):
    """(T,B,1,S,S) frames from sprites (N,D,D), ids (B,ND) int32 and pos (B,ND,T,2) int32 (dvg_moving_mnist_compose)."""
    _dev_f32(sprites, "moving_mnist_compose.sprites")
    if ids.dtype != torch.int32 or pos.dtype != torch.int32 or not ids.is_cuda or not pos.is_cuda:
        raise RuntimeError("moving_mnist_compose: ids / pos must be int32 device tensors")
    ids, pos, sprites = ids.contiguous(), pos.contiguous(), sprites.contiguous()
    b, nd = ids.shape
    if tuple(pos.shape) != (b, nd, seq_len, 2):
        raise RuntimeError(f"moving_mnist_compose: pos shape {tuple(pos.shape)}")
    out = torch.empty((seq_len, b, 1, image_size, image_size), device=sprites.device, dtype=torch.float32)
    check(lib().dvg_moving_mnist_compose(_p(sprites), _p(ids), _p(pos), _p(out), sprites.shape[0], seq_len, b, nd,
                                         image_size, sprites.shape[1], _stream()), "dvg_moving_mnist_compose")
    return out


def clip_gather(pool, first, T, C):
    """(T,B,C,H,W) float32 clips = pool[first[b] + t] / 255 out of a device frame pool (n_frames,H,W,pool_c) uint8
    (dvg_clip_gather_u8): what utils.normalize_data makes of the KTH / BAIR / UCF loaders' batches.  `first`: the B pool
    indices of the clips' first frames - host int64 values (checked against the pool here, then uploaded on the current
    stream) or an int64 device tensor (the kernel clamps what it reads)."""
    if not pool.is_cuda or pool.dtype != torch.uint8 or pool.dim() != 4 or not pool.is_contiguous():
        raise RuntimeError("clip_gather: pool must be a contiguous (n_frames,H,W,pool_c) uint8 GPU tensor - no CPU fallback")
    n, h, w, pc = pool.shape
    if not (isinstance(first, torch.Tensor) and first.is_cuda):
        first = torch.as_tensor(first)
        if first.dtype != torch.int64 or first.dim() != 1 or first.numel() == 0:
            raise RuntimeError("clip_gather: first must be a non-empty 1-D int64 sequence")
        if T < 1 or int(first.min()) < 0 or int(first.max()) + T > n:
            raise RuntimeError(f"clip_gather: clips of {T} frames at [{int(first.min())}, {int(first.max())}] leave the "
                               f"pool of {n} frames")
        first = first.to(pool.device)
    if first.dtype != torch.int64 or first.dim() != 1 or not first.is_contiguous() or first.device != pool.device:
        raise RuntimeError("clip_gather: first must be a contiguous 1-D int64 tensor on the pool's device")
    b = first.shape[0]
    out = torch.empty((max(T, 0), b, C, h, w), device=pool.device, dtype=torch.float32)
    _run("clip_gather", 0.0, float(T * b * h * w * pc) + 4.0 * out.numel(), lib().dvg_clip_gather_u8, _p(pool), _p(first),
         _p(out), n, T, b, C, h, w, pc, _stream())
    return out


CLIP_MAX_SHIFT = 16     # DVG_CLIP_MAX_SHIFT of clips.hip: the kernel clamps dy / dx to it


def clip_gather_aug(pool, first, geom, photo, T, C):
    """`clip_gather` with per-clip augmentation (dvg_clip_gather_aug_u8): geom (B,4) int32 = [hflip, reverse, dy, dx], photo
    (B,2) float32 = [gain, bias]; out[t,b,c,y,x] = clip(gain * v + bias, 0, 1) of v = pool[first[b] + ts, sy, sx, c] / 255 with
    ts = T-1-t under reverse, sx from W-1-x under hflip, and the shift (dy, dx) with edge replication.  Identity parameters give
    clip_gather's bits.  Host arrays are range-checked here (first against the pool, |dy|, |dx| <= 16, finite gain / bias); when
    all three are host arrays they travel as ONE buffer - a batch stays one upload and one launch.  An int64 / int32 / float32
    device tensor is passed through: the kernel clamps what it reads."""
    if not pool.is_cuda or pool.dtype != torch.uint8 or pool.dim() != 4 or not pool.is_contiguous():
        raise RuntimeError("clip_gather_aug: pool must be a contiguous (n_frames,H,W,pool_c) uint8 GPU tensor - no CPU fallback")
    n, h, w, pc = pool.shape

    def on_device(t):
        return isinstance(t, torch.Tensor) and t.is_cuda

    def host_array(t):      # numpy arrays, CPU tensors and sequences alike, without a copy where there is an array already
        return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t)
    # the checks of host arrays run in numpy: a handful of one-element torch ops per batch cost more than the launch
    host = {}
    if not on_device(first):
        f = host_array(first)
        if f.dtype != np.int64 or f.ndim != 1 or f.size == 0:
            raise RuntimeError("clip_gather_aug: first must be a non-empty 1-D int64 sequence")
        if T < 1 or int(f.min()) < 0 or int(f.max()) + T > n:
            raise RuntimeError(f"clip_gather_aug: clips of {T} frames at [{int(f.min())}, {int(f.max())}] leave the pool of "
                               f"{n} frames")
        host["first"] = f
    if not on_device(geom):
        g = host_array(geom)
        if g.dtype != np.int32 or g.ndim != 2 or g.shape[1] != 4 or g.size == 0:
            raise RuntimeError("clip_gather_aug: geom must be a non-empty (B,4) int32 array [hflip, reverse, dy, dx]")
        if int(g[:, 2:].min()) < -CLIP_MAX_SHIFT or int(g[:, 2:].max()) > CLIP_MAX_SHIFT:
            raise RuntimeError(f"clip_gather_aug: a shift (dy, dx) beyond +-{CLIP_MAX_SHIFT} pixels")
        host["geom"] = g
    if not on_device(photo):
        ph = host_array(photo)
        if ph.dtype != np.float32 or ph.ndim != 2 or ph.shape[1] != 2 or ph.size == 0:
            raise RuntimeError("clip_gather_aug: photo must be a non-empty (B,2) float32 array [gain, bias]")
        if not np.isfinite(ph).all():
            raise RuntimeError("clip_gather_aug: gain / bias must be finite")
        host["photo"] = ph
    if len(host) == 3:      # one buffer, one upload: first (8 B bytes) | geom (16 B) | photo (8 B), each part 8-byte aligned
        a, b_ = host["first"].nbytes, host["first"].nbytes + host["geom"].nbytes
        buf = np.empty(b_ + host["photo"].nbytes, np.uint8)
        buf[:a], buf[a:b_], buf[b_:] = (host[k].reshape(-1).view(np.uint8) for k in ("first", "geom", "photo"))
        packed = torch.from_numpy(buf).to(pool.device)
        first, geom, photo = packed[:a].view(torch.int64), packed[a:b_].view(torch.int32).view(-1, 4), \
            packed[b_:].view(torch.float32).view(-1, 2)
    else:
        first, geom, photo = (torch.from_numpy(host[k]).to(pool.device) if k in host else t
                              for k, t in (("first", first), ("geom", geom), ("photo", photo)))
    if first.dtype != torch.int64 or first.dim() != 1 or not first.is_contiguous() or first.device != pool.device:
        raise RuntimeError("clip_gather_aug: first must be a contiguous 1-D int64 tensor on the pool's device")
    b = first.shape[0]
    if geom.dtype != torch.int32 or tuple(geom.shape) != (b, 4) or not geom.is_contiguous() or geom.device != pool.device:
        raise RuntimeError(f"clip_gather_aug: geom must be a contiguous ({b},4) int32 tensor on the pool's device")
    if photo.dtype != torch.float32 or tuple(photo.shape) != (b, 2) or not photo.is_contiguous() or photo.device != pool.device:
        raise RuntimeError(f"clip_gather_aug: photo must be a contiguous ({b},2) float32 tensor on the pool's device")
    out = torch.empty((max(T, 0), b, C, h, w), device=pool.device, dtype=torch.float32)
    _run("clip_gather_aug", 0.0, float(T * b * h * w * pc) + 4.0 * out.numel(), lib().dvg_clip_gather_aug_u8, _p(pool), _p(first),
         _p(geom), _p(photo), _p(out), n, T, b, C, h, w, pc, _stream())
    return out


def mnist_scale_u8(raw, out_size=32, tables=None):
    """(n,out,out) uint8 = Pillow's bilinear `resize((out, out))` of raw (n,s,s) uint8, bit for bit (dvg_mnist_scale_u8):
    `transforms.Scale(32)` on a split's MNIST digits, once.  The coefficient tables come from dvg_amd/mnist.py and are uploaded
    here; `tables` = (xmin, coef) of mnist.resize_tables already on the device spares the upload (a graph capture)."""
    from .. import mnist
    if not raw.is_cuda or raw.dtype != torch.uint8 or raw.dim() != 3 or raw.shape[1] != raw.shape[2] or not raw.is_contiguous() \
            or raw.shape[0] == 0:
        raise RuntimeError("mnist_scale_u8: raw must be a contiguous non-empty (n,s,s) uint8 GPU tensor - no CPU fallback")
    n, s, _ = raw.shape
    if s > out_size or out_size > 64:
        raise RuntimeError(f"mnist_scale_u8: {s} -> {out_size}: only up-scaling to at most 64 is restated")
    if tables is None:
        tables = [torch.from_numpy(t).to(raw.device) for t in mnist.resize_tables(s, out_size)]
    xmin, coef = tables
    if any(t.dtype != torch.int32 or t.device != raw.device or not t.is_contiguous() for t in tables) or \
            tuple(xmin.shape) != (out_size,) or tuple(coef.shape) != (out_size, mnist.TAPS):
        raise RuntimeError("mnist_scale_u8: tables must be int32 (out,) and (out,3) tensors on raw's device")
    out = torch.empty((n, out_size, out_size), device=raw.device, dtype=torch.uint8)
    _run("mnist_scale_u8", 0.0, float(raw.numel() + out.numel()), lib().dvg_mnist_scale_u8, _p(raw), _p(out), n, s, out_size,
         _p(xmin), _p(coef), _stream())
    return out


def moving_mnist_compose_u8(sprites, ids, pos, seq_len, image_size):
    """(T,B,1,S,S) float32 frames from a uint8 digit pool (N,D,D), ids (B,ND) and pos (B,ND,T,2) = (sy,sx), int32
    (dvg_moving_mnist_compose_u8).  ids / pos: host arrays (checked against the pool and the canvas here, then uploaded on the
    current stream) or int32 device tensors (the kernel clamps ids and bounds-checks every access against pos)."""
    if not sprites.is_cuda or sprites.dtype != torch.uint8 or sprites.dim() != 3 or sprites.shape[1] != sprites.shape[2] \
            or not sprites.is_contiguous():
        raise RuntimeError("moving_mnist_compose_u8: sprites must be a contiguous (N,D,D) uint8 GPU tensor - no CPU fallback")
    n, d, _ = sprites.shape
    if not (isinstance(ids, torch.Tensor) and ids.is_cuda):
        ids, pos = torch.as_tensor(ids), torch.as_tensor(pos)
        if ids.numel() == 0 or pos.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= n:
            raise RuntimeError(f"moving_mnist_compose_u8: ids outside the pool of {n} digits")
        if int(pos.min()) < 0 or int(pos.max()) > image_size - d:
            raise RuntimeError(f"moving_mnist_compose_u8: pos outside [0, {image_size - d}]: a digit would leave the canvas")
        if ids.dtype != torch.int32 or pos.dtype != torch.int32:
            raise RuntimeError("moving_mnist_compose_u8: ids / pos must be int32")
        ids, pos = ids.to(sprites.device), pos.to(sprites.device)
    if ids.dtype != torch.int32 or not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32 or ids.dim() != 2 \
            or ids.device != sprites.device or pos.device != sprites.device:
        raise RuntimeError("moving_mnist_compose_u8: ids (B,ND) / pos must be int32 tensors on the pool's device")
    ids, pos = ids.contiguous(), pos.contiguous()
    b, nd = ids.shape
    if tuple(pos.shape) != (b, nd, seq_len, 2):
        raise RuntimeError(f"moving_mnist_compose_u8: pos shape {tuple(pos.shape)}")
    out = torch.empty((seq_len, b, 1, image_size, image_size), device=sprites.device, dtype=torch.float32)
    check(lib().dvg_moving_mnist_compose_u8(_p(sprites), _p(ids), _p(pos), _p(out), n, seq_len, b, nd, image_size, d,
                                            _stream()), "dvg_moving_mnist_compose_u8")
    return out
