"""GPU: dvg_frame_mosaic (ops.frame_mosaic) against the CPU restatement of the reference's figure code (tests/viz_ref.py,
itself pinned to the reference by tests/golden/reference_viz.npz and tests/test_viz_host.py): BIT-EQUAL uint8 mosaics for the
three layouts, both byte conversions, with and without label masks, row widths that are no multiple of 4 or 16 bytes; the
selection of `best` / `picks` on the device; the entry points' files.  One process, small shapes."""
import os

import numpy as np
import pytest
import torch

from dvg_amd import ops, viz
from dvg_amd import utils as dvg_utils
from tests import viz_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(layout, sources, best=None, picks=None, masks=None, quant=None, table=None):
    """ops.frame_mosaic on a layout, every operand uploaded here; masks: a host (n, lh, lw) array or None."""
    srcs = [None if s is None else s.to(DEV) for s in sources]
    nc = next(s for s in srcs if s is not None).shape[-3]
    cells = torch.from_numpy(np.ascontiguousarray(layout.table if table is None else table).reshape(-1)).to(DEV)
    return ops.frame_mosaic(
        srcs, cells, nc=nc, H=layout.H, W=layout.W, F=layout.F, R=layout.R, Cc=layout.Cc, cell_h=layout.cell_h,
        cell_w=layout.cell_w, pad_y=layout.pad_y, pad_x=layout.pad_x, oy=layout.oy, ox=layout.ox,
        best=None if best is None else best.to(DEV),
        picks=None if picks is None else torch.from_numpy(np.ascontiguousarray(picks, dtype=np.int32)).to(DEV),
        labels=None if masks is None else torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint8)).to(DEV),
        quant=layout.quant if quant is None else quant).cpu().numpy()


def case(nc, H, B, T=6, S=3, seed=0):
    x = viz_ref.seeded(1000 + seed, T, B, nc, H, H)
    post = viz_ref.seeded(2000 + seed, T, B, nc, H, H)
    samples = viz_ref.seeded(3000 + seed, S, T, B, nc, H, H)
    best = torch.from_numpy(np.random.RandomState(seed).randint(0, S, size=B)).to(torch.int64)
    best[:2] = S - 1                                                                     # repeats
    return x, post, samples, best


def expect(layout, sources, best, picks, masks, quant):
    old = layout.quant
    layout.quant = quant
    try:
        return viz_ref.render_layout(layout, sources, best, picks, masks)
    finally:
        layout.quant = old


@pytest.mark.parametrize("quant", [viz.QUANT_TRUNC, viz.QUANT_NEAREST])
@pytest.mark.parametrize("nc,H,B", [(1, 64, 4), (3, 64, 4), (1, 128, 4), (3, 128, 4), (1, 64, 50), (3, 64, 50)])
def test_three_layouts_are_bit_equal_to_the_restatement(nc, H, B, quant):
    x, post, samples, best = case(nc, H, B)
    T, S = x.shape[0], samples.shape[0]
    n_past = 2
    rows = min(B, 5)
    # make_gifs: row bytes 6 * 66 * 3 = 1188 (a multiple of 4, not of 16) at 64 x 64
    lay = viz.make_gifs_layout(T, n_past, B, H, rows=rows)
    picks = viz.random_picks(21, rows, 3, S)
    synth = (np.random.RandomState(9).rand(6, lay.cell_h - 3, lay.cell_w - 5) < 0.15).astype(np.uint8)
    font = viz.render_labels(lay.labels, lay.cell_h, lay.cell_w)        # None without Pillow
    for masks in (None, synth, font):
        got = run(lay, [x, post, samples], best, picks, masks, quant)
        ref = expect(lay, [x, post, samples], best, picks, masks, quant)
        assert got.shape == ref.shape == (rows * T, H + 32, 6 * (H + 2), 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref), ("make_gifs", np.argwhere(got != ref)[:4])
    # plot: PNG rows of T * H + T - 1 pixels, GIF rows of 6 * H + 5: 389 * 3 = 1167 bytes at 64 x 64, no multiple of 4
    png_l, gif_l = viz.plot_layout(T, B, H)
    p4 = viz.random_picks(22, min(B, 10), 4, S)
    for name, l in (("png", png_l), ("gif", gif_l)):
        got = run(l, [x, None, samples], best, p4, None, quant)
        ref = expect(l, [x, None, samples], best, p4, None, quant)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, np.argwhere(got != ref)[:4])
    assert (gif_l.grid_w * 3) % 4 != 0
    rec = viz.plot_rec_layout(T, H, index=B - 1, B=B)
    got = run(rec, [x], quant=quant)
    assert np.array_equal(got, expect(rec, [x], None, None, None, quant))


@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("nc", [1, 3])
def test_row_bytes_of_66_times_3_times_k_and_partial_last_group(nc, k):
    """k bordered 64 x 64 cells side by side: 198 k bytes a row (k = 1, 3, 5: no multiple of 4; k = 2: of 4, not of 16), through
    the reference-style helpers; and single frames whose pixel count is no multiple of four (the byte-wise tail)."""
    imgs = [viz_ref.seeded(400 + i, nc, 64, 64) for i in range(k)]
    colours = ['green', 'red', None, 'red', 'green']
    cells = [dvg_utils.add_border(im.to(DEV), colours[i]) for i, im in enumerate(imgs)]
    ref_cells = [viz_ref.add_border(im, colours[i]) for i, im in enumerate(imgs)]
    for quant in (viz.QUANT_TRUNC, viz.QUANT_NEAREST):
        got = dvg_utils.image_tensor(cells, padding=0).bytes(quant).cpu().numpy()
        ref = viz_ref.to_bytes(viz_ref.image_tensor(ref_cells, padding=0), quant)
        assert got.shape == (96, 66 * k, 3) and np.array_equal(got, ref)
    for h, w in ((5, 7), (3, 3), (1, 1), (9, 11)):                        # 35, 9, 1, 99 pixels
        im = viz_ref.seeded(500 + h, nc, h, w)
        got = dvg_utils.image_tensor([im.to(DEV)], padding=1).bytes(viz.QUANT_NEAREST).cpu().numpy()
        assert np.array_equal(got, viz_ref.to_bytes(im, viz.QUANT_NEAREST)), (h, w)


def test_ties_clamp_and_contraction():
    """Values below 0, above 1, 0.7f (0.7f * 255 = 178.5 exactly in fp32) and every k / 255 and (k + 0.5) / 255: a fused
    multiply-add, a missing clamp or another rounding would change bytes."""
    k = torch.arange(256, dtype=torch.float32)
    vals = torch.cat([k / 255, (k + 0.5) / 255, torch.tensor([0.7, -0.5, -0.0, 1.5, 1.0, 0.999999, 1e-9, 0.5]),
                      viz_ref.seeded(77, 504).reshape(-1)])
    vals = vals[:1024].reshape(1, 1, 32, 32)
    lay = viz.plot_rec_layout(1, 32)
    for quant in (viz.QUANT_TRUNC, viz.QUANT_NEAREST):
        got = run(lay, [vals.unsqueeze(0)], quant=quant)[0]
        ref = viz_ref.to_bytes(vals[0], quant)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]
    flat = run(lay, [vals.unsqueeze(0)], quant=viz.QUANT_NEAREST)[0][:, :, 0].reshape(-1)
    assert flat[512] == 179                                               # 0.7f: 178.5 + 0.5, not fma(0.7f, 255, 0.5)


def test_kernel_equals_the_reference_outputs_directly():
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_viz.npz"))
    for name in viz_ref.GOLDEN_CASES:
        inputs, padding = viz_ref.golden_inputs(name)
        dev_in = [[t.to(DEV) for t in row] for row in inputs] if isinstance(inputs[0], list) else [t.to(DEV) for t in inputs]
        for quant in (viz.QUANT_TRUNC, viz.QUANT_NEAREST):
            got = dvg_utils.image_tensor(dev_in, padding).bytes(quant).cpu().numpy()
            ref = viz_ref.to_bytes(torch.from_numpy(g[name]), quant)
            assert got.shape == ref.shape and np.array_equal(got, ref), (name, quant)
    frame = viz_ref.golden_text_frame()
    cell = dvg_utils.draw_text_tensor(dvg_utils.add_border(frame[0:1, 1:17, 1:17].to(DEV).contiguous(), 'red'), "")
    got = dvg_utils.image_tensor([cell], padding=0).bytes(viz.QUANT_TRUNC).cpu().numpy()
    assert np.array_equal(got, np.rint(g["draw_text_empty"] * 255).astype(np.uint8).transpose(1, 2, 0))


def test_selection_happens_on_the_device_without_a_read_back():
    x, post, samples, best = case(1, 64, 4, seed=3)
    T, B, S = x.shape[0], x.shape[1], samples.shape[0]
    lay = viz.make_gifs_layout(T, 2, B, 64, rows=B)
    picks = viz.random_picks(5, B, 3, S)
    on_device = run(lay, [x, post, samples], best, picks)
    # the same figure with the indices resolved on the host: every selected cell becomes a plain image number
    tab = lay.table.copy().reshape(-1, 8)
    for e in tab:
        if e[3] != viz.SEL_NONE:
            s = int(best[e[4]]) if e[3] == viz.SEL_BEST else int(picks[e[4]][e[5]])
            e[1], e[2], e[3] = e[1] + s * e[2], 0, viz.SEL_NONE
    assert np.array_equal(on_device, run(lay, [x, post, samples], table=tab.reshape(lay.table.shape)))
    other = best.clone()
    other[0] = (best[0] + 1) % S
    assert not np.array_equal(on_device, run(lay, [x, post, samples], other, picks))
    # operands uploaded first; the call itself must not synchronise (no index is read back)
    srcs = [t.to(DEV) for t in (x, post, samples)]
    cells, masks = lay.upload(DEV)
    best_d, picks_d = best.to(DEV), torch.from_numpy(picks).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.frame_mosaic(srcs, cells, nc=1, H=64, W=64, F=lay.F, R=1, Cc=6, cell_h=96, cell_w=66, oy=1, ox=1,
                               best=best_d, picks=picks_d, labels=masks, quant=viz.QUANT_TRUNC)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    font = viz.render_labels(lay.labels, 96, 66)
    assert np.array_equal(out.cpu().numpy(), viz_ref.render_layout(lay, [x, post, samples], best, picks, font))


def test_bad_table_entries_draw_the_background_only():
    """The kernel checks what it reads from device memory: out-of-range sources, image numbers, indices and labels leave the
    cell's background (and never read outside a source)."""
    x, post, samples, best = case(1, 64, 4, seed=4)
    lay = viz.make_gifs_layout(x.shape[0], 2, 4, 64)
    picks = viz.random_picks(5, 1, 3, 3)
    tab = lay.table.copy()
    tab[0, 0, 0, 0] = 7                 # no such source
    tab[0, 0, 1, 1] = 10 ** 6           # image number beyond the source
    tab[0, 0, 2, 4] = 99                # best[99]
    tab[0, 0, 3, 5] = 3                 # picks[0][3]
    tab[0, 0, 4, 0] = -1
    bad_best = best.clone()
    bad_best[0] = 10 ** 9
    got = run(lay, [x, post, samples], bad_best, picks, table=tab)
    ref = viz_ref.render_layout(lay, [x, post, samples], best, picks)
    for c in range(5):
        cell = got[0, :, c * 66:(c + 1) * 66]
        assert (cell[:, :, 2] == 0).all() and len(np.unique(cell[:, :, 0])) == 1 and len(np.unique(cell[:, :, 1])) == 1, c
    assert np.array_equal(got[0, :, 5 * 66:], ref[0, :, 5 * 66:])
    assert np.array_equal(got[1][:, :66], ref[1][:, :66])
    assert (got[1][:, 2 * 66:3 * 66] == np.array([0, 178, 0], dtype=np.uint8)).all()          # best[0] = 10^9: green background only


def _decode_gif(path):
    from PIL import Image
    im = Image.open(path)
    frames = []
    for f in range(im.n_frames):
        im.seek(f)
        frames.append(np.asarray(im.convert("RGB")))
    return frames


def test_generate_frames_writes_gifs_and_pngs_and_leaves_the_tensors_alone(tmp_path):
    import generate_frames
    base = ["--synthetic_ckpt", "--model", "dcgan", "--dataset", "smmnist", "--batch_size", "4", "--n_past", "2", "--nsample",
            "3", "--nbatches", "1"]
    with_img, without = str(tmp_path / "a"), str(tmp_path / "b")
    # main() builds the synthetic checkpoint BEFORE it seeds torch (the weights come from the generator's state at the call)
    torch.manual_seed(4)
    generate_frames.main(base + ["--n_eval", "6", "--log_dir", with_img])
    torch.manual_seed(4)
    generate_frames.main(base + ["--n_eval", "6", "--log_dir", without, "--no_images"])
    pa, pb = (torch.load(os.path.join(d, "gen", "sample_lstm_0.pt")) for d in (with_img, without))
    assert sorted(pa) == sorted(pb)
    for key in pa:
        assert torch.equal(pa[key], pb[key]), key
    gif = os.path.join(with_img, "gen", "sample_lstm_0.gif")
    assert not os.path.exists(os.path.join(without, "gen", "sample_lstm_0.gif"))
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert not os.path.exists(gif)                  # warned and skipped
    else:
        frames = _decode_gif(gif)
        assert len(frames) == 6 and frames[0].shape == (96, 6 * 66, 3)
        # green, then red borders (grey levels + border colours may exceed 256 colours: Pillow then quantises, so: close to)
        assert np.abs(frames[0][0, 0].astype(int) - (0, 178, 0)).max() <= 12
        assert np.abs(frames[5][0, 66 + 2].astype(int) - (178, 0, 0)).max() <= 12
    # the trigger figure: one PNG per index, every third frame in a row
    trig = str(tmp_path / "t")
    generate_frames.main(base + ["--n_eval", "15", "--log_dir", trig, "--gp_trigger", "--trigger_indices", "2"])
    res = torch.load(os.path.join(trig, "gen", "gp_trigger_0.pt"))
    from tests.test_viz_host import decode_png
    for r in res[:2]:
        png = decode_png(os.path.join(trig, "gen", "recursive_generation", str(r["index"]), "heuristic_gp_trigger_1_0.png"))
        assert np.array_equal(png, viz_ref.plot_rec_reference(r["frames"].unsqueeze(1), 0))


def test_trainer_plot_hook_writes_the_png_and_gif(tmp_path):
    from tests.test_gpu_rollouts import _trainer
    import utils
    from dvg_amd.data import SyntheticMovingMNIST
    from tests.test_viz_host import decode_png
    B, n_eval = 4, 12
    tr, o = _trainer("dcgan", B, 2, 3, n_eval)
    tr.frame_predictor.eval(), tr.gp_layer.eval(), tr.likelihood.eval()
    ds = SyntheticMovingMNIST(seq_len=n_eval, image_size=64, seed=5)
    x, _ = utils.normalize_data(o, torch.cuda.FloatTensor, ds.batch(B))
    gen, best = tr.plot(x, 0)
    g0, b0 = gen.clone(), best.clone()
    png, gif = tr.write_plot(x, gen, best, 0, str(tmp_path))
    assert torch.equal(gen, g0) and torch.equal(best, b0)
    picks = viz.random_picks(o.seed, B, 4, gen.shape[0])                   # the trainer's private stream, first draw
    gt = torch.stack(list(x[:n_eval])).cpu()
    ref_png, ref_gif = viz_ref.plot_reference(gt, gen.cpu(), best.cpu(), picks, n_eval)
    assert os.path.basename(png) == "sample_0.png" and np.array_equal(decode_png(png), ref_png)
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert gif is None
        return
    frames = _decode_gif(gif)
    assert len(frames) == n_eval and frames[0].shape == ref_gif[0].shape
    if len(np.unique(np.concatenate([f.reshape(-1, 3) for f in ref_gif]), axis=0)) <= 256:   # the exact-palette condition
        assert np.array_equal(frames[0], ref_gif[0])
