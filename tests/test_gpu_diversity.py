"""GPU: dvg_pairwise_frame_mse (ops.pairwise_frame_mse), utils.sample_diversity and make_gifs(diversity=True) against the fp64
differences of tests/diversity_ref.py.

Bar: every entry within 2e-5 RELATIVE of the reference, no absolute slack, zeros exactly zero.  It is derived, not measured: the
kernel sums fp32 squares of fp32 differences in chunks of at most 256 consecutive elements and adds the chunks in fp64, and a
sum of n non-negative fp32 terms, each a rounded square of a rounded difference, is within about (n + 4) 2^-24 of exact - (256
+ 4) 2^-24 = 1.6e-5, rounded up.  Seen on the MI355X (worst entry / bar): 0.021 at S = 100, D = 121
(4.2e-7 relative), 0.015 and less in the other eight parity cases, 0.003 on the returned samples of make_gifs."""
import functools

import numpy as np
import pytest
import torch

from tests import diversity_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 2e-5
T, B, LO, HI = 3, 2, 1, 3            # a step range inside the tensor: a wrong base or stride shows


def _close(got, want, what):
    """got: fp32 device tensor; want: fp64 array.  Relative everywhere; where the reference is 0 the result is 0."""
    g = got.cpu().numpy().astype(np.float64)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    zero = want == 0
    assert np.array_equal(g[zero], want[zero]), what
    ratio = (np.abs(g[~zero] - want[~zero]) / want[~zero]).max() / RTOL if (~zero).any() else 0.0
    print(f"{what}: worst entry / bar {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


@functools.lru_cache(maxsize=None)
def _case(s, c, h, w):
    """Seeded uniform [0, 1) samples (S,T,B,C,H,W), on the device, and their fp64 matrix over [LO, HI); computed once."""
    x = np.random.RandomState(1000 * s + c * h + w).random_sample((s, T, B, c, h, w)).astype(np.float32)
    return torch.from_numpy(x).to(DEV), ref.pairwise_frame_mse(x, LO, HI)


def _op(x, lo=None, hi=None):
    from dvg_amd import ops
    out = ops.pairwise_frame_mse(x, lo, hi)
    torch.cuda.synchronize()
    return out


# S <= 32 runs 32-row tiles, above that 64-row tiles (S = 100: two tiles, three tile blocks); D = 121 takes the element loads
# (not a multiple of 4) and ends inside a slab, the others the 16-byte loads
@pytest.mark.parametrize("s,c,h,w", [(1, 1, 11, 11), (2, 1, 11, 11), (5, 1, 11, 11), (33, 1, 11, 11), (100, 1, 11, 11),
                                     (5, 1, 64, 64), (33, 1, 64, 64), (33, 3, 64, 64), (5, 3, 128, 128)])
def test_parity_with_fp64(s, c, h, w):
    x, want = _case(s, c, h, w)
    got = _op(x, LO, HI)
    assert got.shape == (HI - LO, B, s, s) and got.dtype == torch.float32
    _close(got, want, f"S {s} frame {c}x{h}x{w}")


def test_exact_zeros_and_symmetry():
    x = _case(5, 1, 64, 64)[0].clone()
    x[3] = x[0]
    out = _op(x)
    assert torch.equal(out[..., 0, 3], torch.zeros_like(out[..., 0, 3])) and torch.equal(out[..., 3, 0], out[..., 0, 3])
    off = ~torch.eye(5, dtype=torch.bool, device=DEV)
    off[0, 3] = off[3, 0] = False
    assert bool((out[..., off] > 0).all())
    assert torch.equal(torch.diagonal(out, dim1=-2, dim2=-1), torch.zeros(T, B, 5, device=DEV))
    x33 = _case(33, 1, 64, 64)[0]
    out = _op(x33)
    assert torch.equal(out.view(torch.int32), out.transpose(-1, -2).contiguous().view(torch.int32))
    assert torch.equal(torch.diagonal(out, dim1=-2, dim2=-1), torch.zeros(T, B, 33, device=DEV))


def test_near_identical_pair_keeps_its_difference():
    """Two samples that differ in one pixel by 2^-20 (0.5 against 0.5 + 2^-20, both exact in fp32): the entry is (2^-20)^2 / D.
    A Gram form gets 0 or noise here: |a|^2 is about D / 3 and its fp32 rounding alone exceeds 2^-40 by many orders."""
    for shape in ((1, 11, 11), (1, 64, 64)):
        d = int(np.prod(shape))
        x = _case(5, *shape)[0][:2].clone()
        x[1] = x[0]
        x[0, :, :, 0, 5, 7] = 0.5
        x[1, :, :, 0, 5, 7] = 0.5 + 2.0 ** -20
        out = _op(x)
        want = np.zeros((T, B, 2, 2))
        want[..., 0, 1] = want[..., 1, 0] = (2.0 ** -40) / d
        _close(out, want, f"one pixel by 2^-20, D {d}")


def test_two_calls_give_the_same_bits():
    x = torch.from_numpy(np.random.RandomState(7).random_sample((100, 2, 2, 1, 64, 64)).astype(np.float32)).to(DEV)
    a, b = _op(x), _op(x)
    assert a.shape == (2, 2, 100, 100) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("s,c,h,w", [(5, 1, 11, 11), (33, 1, 64, 64)])
def test_step_range_equals_a_contiguous_copy(s, c, h, w):
    x = _case(s, c, h, w)[0]
    part = x[:, LO:HI].contiguous()
    assert torch.equal(_op(x, LO, HI).view(torch.int32), _op(part).view(torch.int32))
    assert torch.equal(_op(x)[LO:HI].view(torch.int32), _op(part).view(torch.int32))


def test_nan_stays_in_its_row_and_column():
    x = _case(5, 1, 64, 64)[0].clone()
    clean = _op(x)
    x[2, 0, 1, 0, 9, 9] = float("nan")                 # sample 2 of frame (step 0, row 1) = frame 1
    out = _op(x)
    hit = torch.zeros(T, B, 5, 5, dtype=torch.bool, device=DEV)
    hit[0, 1, 2, :] = hit[0, 1, :, 2] = True
    hit[0, 1, 2, 2] = False
    assert bool(torch.isnan(out[hit]).all())
    assert torch.equal(out[~hit].view(torch.int32), clean[~hit].view(torch.int32))
    assert float(out[0, 1, 2, 2]) == 0.0


def test_errors_raise_before_any_launch():
    from dvg_amd import ops
    x = _case(5, 1, 11, 11)[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pairwise_frame_mse(x.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        ops.pairwise_frame_mse(x.double())
    with pytest.raises(RuntimeError, match="S,T,B,C,H,W"):
        ops.pairwise_frame_mse(x[0])
    for lo, hi in ((2, 2), (2, 1), (0, T + 1), (-1, 2)):
        with pytest.raises(RuntimeError, match="step range"):
            ops.pairwise_frame_mse(x, lo, hi)


def _check_diversity(dv, samples, n_past, what):
    """utils.sample_diversity's dict against the same quantities from the fp64 matrix of the same samples."""
    m = ref.pairwise_frame_mse(samples.cpu().numpy(), n_past, samples.shape[1])
    pair, psnr, distinct = ref.diversity(m)
    assert dv["pair_mse"].dtype == torch.float64 and dv["pair_psnr"].dtype == torch.float64
    assert dv["distinct"].dtype == torch.int64 and dv["matrix_last"].dtype == torch.float32
    _close(dv["matrix_last"], m[-1], what + " matrix_last")
    got = dv["pair_mse"].cpu().numpy()
    assert got.shape == pair.shape
    np.testing.assert_allclose(got, pair, rtol=RTOL, atol=0)
    assert np.array_equal(got == 0, pair == 0)
    gp = dv["pair_psnr"].cpu().numpy()
    fin = np.isfinite(psnr)
    assert np.array_equal(gp[~fin], psnr[~fin])
    np.testing.assert_allclose(gp[fin], psnr[fin], rtol=0, atol=10 * np.log10(1 + RTOL))
    assert np.array_equal(dv["distinct"].cpu().numpy(), distinct)
    return m


def test_sample_diversity_against_the_fp64_matrix():
    import utils
    x = _case(33, 1, 11, 11)[0].clone()
    for group in ((0, 4, 9), (1, 2), (5, 30, 31, 32)):   # three groups of repeated samples: 33 - 2 - 1 - 3 different frames
        for s in group[1:]:
            x[s] = x[group[0]]
    x[:, 2] = x[0:1, 2]                                   # the last step: every sample the same
    dv = utils.sample_diversity(x, 1)
    torch.cuda.synchronize()
    assert dv["pair_mse"].shape == (B, T - 1) and dv["matrix_last"].shape == (B, 33, 33)
    _check_diversity(dv, x, 1, "three groups")
    assert dv["distinct"].tolist() == [[27, 1]] * B
    assert bool((dv["pair_mse"][:, 1] == 0).all()) and bool(torch.isposinf(dv["pair_psnr"][:, 1]).all())
    one = utils.sample_diversity(x[:1], 1)
    assert bool((one["pair_mse"] == 0).all()) and bool(torch.isposinf(one["pair_psnr"]).all())
    assert one["distinct"].tolist() == [[1, 1]] * B and one["matrix_last"].shape == (B, 1, 1)


# ---- make_gifs ---------------------------------------------------------------------------------------------------------------
# rollout._predict_from: the loop step i decodes frame i itself, and sample_from swaps the latent for a GP draw at i % 15 == 0.  With
# n_past = 13 and n_eval = 17 the predicted frames are 13 ... 16 and the only trigger step is 15: frames 13 and 14 (predicted
# steps 0, 1) are the same computation for every sample, frame 15 (predicted step 2) is the first that a draw changes.
GB, N_PAST, N_EVAL, NS, FIRST = 4, 13, 17, 4, 2


def _generator(inflight):
    import generate_frames
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", str(GB), "--model", "dcgan",
                                                     "--n_past", str(N_PAST), "--n_eval", str(N_EVAL),
                                                     "--inflight", str(inflight)])
    torch.manual_seed(5100)
    return generate_frames.Generator(opt, generate_frames.synthetic_checkpoint(opt), torch.device(DEV))


@pytest.mark.parametrize("inflight", [0, 2])
def test_make_gifs_diversity(inflight):
    import utils
    from oracle import params
    g = _generator(inflight)
    x = [params.frames(5110 + t, GB, 1, 64).to(DEV) for t in range(N_EVAL)]
    eps = [{15: params.normal(5140 + s, 90, GB).to(DEV)} for s in range(NS)]
    plain = g.make_gifs(x, NS, eps_by_sample=eps)
    assert sorted(plain) == ["best", "posterior", "psnr", "samples", "ssim"]
    plain = {k: v.clone() for k, v in plain.items()}
    res = g.make_gifs(x, NS, eps_by_sample=eps, diversity=True)
    torch.cuda.synchronize()
    assert sorted(res) == ["best", "diversity", "posterior", "psnr", "samples", "ssim"]
    for k in ("samples", "ssim", "psnr", "best", "posterior"):
        assert torch.equal(res[k], plain[k]), k
    dv = res["diversity"]
    assert sorted(dv) == ["distinct", "matrix_last", "pair_mse", "pair_psnr"]
    again = utils.sample_diversity(res["samples"], N_PAST)
    for k in dv:
        assert torch.equal(dv[k], again[k]), k
    _check_diversity(dv, res["samples"], N_PAST, f"make_gifs inflight {inflight}")
    from dvg_amd import ops
    m = ops.pairwise_frame_mse(res["samples"], N_PAST, N_EVAL)
    off = ~torch.eye(NS, dtype=torch.bool, device=DEV)
    assert torch.equal(m[:FIRST], torch.zeros_like(m[:FIRST])) and bool((dv["distinct"][:, :FIRST] == 1).all())
    assert bool((m[FIRST:][..., off] > 0).all()) and bool((dv["distinct"][:, FIRST:] == NS).all())
    assert bool((dv["pair_mse"][:, :FIRST] == 0).all()) and bool((dv["pair_mse"][:, FIRST:] > 0).all())
    if inflight == 0:
        eps[2] = eps[1]
        twin = g.make_gifs(x, NS, eps_by_sample=eps, diversity=True)
        m = ops.pairwise_frame_mse(twin["samples"], N_PAST, N_EVAL)
        assert torch.equal(m[..., 1, 2], torch.zeros_like(m[..., 1, 2]))
        assert bool((twin["diversity"]["distinct"][:, FIRST:] == NS - 1).all())
        assert bool((twin["diversity"]["distinct"][:, :FIRST] == 1).all())
