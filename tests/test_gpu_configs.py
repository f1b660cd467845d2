"""GPU parity at the shapes of BASELINE.json configs C1, C3, C4, C5 (C2 is the bench workload and is covered by
tests/test_gpu_train.py::test_rollout_matches_oracle_rollout and bench.py):
  C1  Moving-MNIST 64x64, B=8, 5-in/5-out, vgg_64 + lstm          (the reference's CPU-runnable case)
  C3  KTH 64x64 nc=1, GP diverse sampling (generate path)           -> same kernels as C2; GP-trigger path here
  C4  BAIR 64x64 nc=3, 16 per GPU, 2-in/10-out, train step          (dcgan_64 / vgg_64, nc = 3)
  C5  UCF 128x128 nc=3, 4 per GPU, 4-in/12-out                      (vgg_128 / dcgan_128)
Sequence lengths are shortened where the CPU oracle would take minutes; shapes per step are the real ones."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dvg_oracle as orc
from oracle import params
from tests.common import YARDSTICK_AT_SCALE, our_module, rel_err, to64, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


LOSS_BAR = 2e-6        # closure VALUES against the oracle: measured r05 <= 1.8e-7 (HIP) / 1.5e-7 (fp32 oracle) against fp64


def _build(family, res, nc, batch, seed):
    mod = our_module(family, res)
    enc, dec = mod.encoder(90, nc), mod.decoder(90, nc)
    esd = params.fill_state_dict(enc.state_dict(), seed)
    dsd = params.fill_state_dict(dec.state_dict(), seed + 1, params.decoder_transposed_keys(dec.state_dict(), family))
    enc.load_state_dict(esd), dec.load_state_dict(dsd)
    from dvg_amd.models.gp_models import GaussianLikelihood, GPRegressionLayer1
    from dvg_amd.models.lstm import lstm
    fp = lstm(90, 90, 256, 2, batch)
    lsd = params.fill_state_dict(fp.state_dict(), seed + 2)
    fp.load_state_dict(lsd)
    gsd, lik = params.gp_state(seed + 3)
    gp, like = GPRegressionLayer1(90), GaussianLikelihood(batch_size=90)
    gp.load_state_dict(gsd), like.load_state_dict(lik)
    return (enc, dec, fp, gp, like), (esd, dsd, lsd, gsd, lik)


def _oracle_fns(family, res, esd, dsd):
    if family == "vgg":
        return (lambda t: orc.vgg_encoder(t, esd, False)), (lambda v, s: orc.vgg_decoder(v, s, dsd, False))
    act = "tanh" if res == 64 else "sigmoid"
    return (lambda t: orc.dcgan_encoder(t, esd, False)), (lambda v, s: orc.dcgan_decoder(v, s, dsd, False, act))


@pytest.mark.parametrize("family,res,nc,batch,n_past,n_eval,last_frame_skip", [
    ("vgg", 64, 1, 8, 5, 10, False),      # C1
    ("dcgan", 64, 3, 16, 2, 6, False),    # C4 shapes (BAIR), shortened horizon
    ("vgg", 64, 3, 16, 2, 4, True),       # C4 with --last_frame_skip
    ("vgg", 128, 3, 4, 2, 4, False),      # C5
    ("dcgan", 128, 3, 4, 4, 7, False),    # C5
])
def test_rollout_parity_at_config_shapes(family, res, nc, batch, n_past, n_eval, last_frame_skip):
    from dvg_amd.rollout import sample_rollout
    mods, (esd, dsd, lsd, gsd, lik) = _build(family, res, nc, batch, 800)
    xs = [params.frames(810 + t, batch, nc, res) for t in range(n_eval)]
    enc_o, dec_o = _oracle_fns(family, res, esd, dsd)
    with torch.no_grad():
        ref = orc.rollout(xs, enc_o, dec_o, lsd, gsd, lik, n_past, n_eval, {}, last_frame_skip=last_frame_skip)
    for m in mods:
        m.to(DEV).eval()
    ours = sample_rollout(*mods, [t.to(DEV) for t in xs], n_past, n_eval, last_frame_skip=last_frame_skip)
    for t in range(n_eval):
        assert ours[t].shape == ref[t].shape
        assert rel_err(ours[t], ref[t]) < 1e-4, (t, rel_err(ours[t], ref[t]))


def test_gp_trigger_generation_bookkeeping():
    """C3: generate_frames.py:249-298 — the variance-threshold trigger.  Integer bookkeeping must be exact:
    the warm-up is 12 steps, triggers can only fire in [12, total), the sliding window keeps 12 values."""
    import argparse
    import generate_frames
    opt = generate_frames.build_parser().parse_args(["--synthetic_ckpt", "--batch_size", "4", "--n_eval", "30",
                                                     "--model", "dcgan"])
    torch.manual_seed(0)
    ckpt = generate_frames.synthetic_checkpoint(opt)
    g = generate_frames.Generator(opt, ckpt, torch.device(DEV))
    xs = [params.frames(900 + t, 4, 1, 64).to(DEV) for t in range(30)]
    res = g.gp_trigger_gen(xs, n_index=2, total=30)
    assert len(res) == 2
    for r in res:
        assert r["frames"].shape == (30, 1, 64, 64)
        assert all(12 <= t < 30 for t in r["triggers"]) and r["triggers"] == sorted(set(r["triggers"]))
        assert bool(torch.isfinite(r["frames"]).all())


@pytest.mark.parametrize("model,width,nc,batch", [("dcgan", 64, 3, 16), ("vgg", 64, 3, 16), ("vgg", 128, 3, 4),
                                                  ("dcgan", 128, 3, 4)])
def test_train_step_at_config_shapes(model, width, nc, batch):
    """C4 / C5 per-GPU training shapes: `train_model` loss against the oracle composition (train.py:200-239; train-mode
    BatchNorm, the family's own final activation), then the fine-tuning closures against theirs."""
    import train
    import utils
    from dvg_amd.data import synthetic_video
    torch.manual_seed(11)
    o = train.options(["--model", model, "--image_width", str(width), "--channels", str(nc), "--batch_size", str(batch),
                       "--n_past", "2", "--n_future", "2", "--dataset", "bair", "--no_save", "--synthetic_data"])
    tr = train.Trainer(o, torch.device(DEV))
    tr.train_mode()
    x, _ = utils.normalize_data(o, torch.cuda.FloatTensor, synthetic_video(batch, 4, nc, width, seed=5))
    tr.gp_layer(torch.zeros(batch, 90, device=DEV))
    cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}  # noqa: E731
    esd, dsd, lsd, gsd, lik = [cpu(m) for m in (tr.encoder, tr.decoder, tr.frame_predictor, tr.gp_layer, tr.likelihood)]
    if model == "vgg":
        enc_o, dec_o = (lambda t: orc.vgg_encoder(t, esd, True)), (lambda v, s: orc.vgg_decoder(v, s, dsd, True))
    else:
        act = "tanh" if width == 64 else "sigmoid"
        enc_o, dec_o = (lambda t: orc.dcgan_encoder(t, esd, True)), (lambda v, s: orc.dcgan_decoder(v, s, dsd, True, act))
    xc = [t.cpu() for t in x]
    e64, d64, l64, g64, k64 = [to64(sd) for sd in (esd, dsd, lsd, gsd, lik)]
    if model == "vgg":
        enc_6, dec_6 = (lambda t: orc.vgg_encoder(t, e64, True)), (lambda v, s: orc.vgg_decoder(v, s, d64, True))
    else:
        enc_6, dec_6 = (lambda t: orc.dcgan_encoder(t, e64, True)), (lambda v, s: orc.dcgan_decoder(v, s, d64, True, act))
    with torch.no_grad():
        ref = float(orc.train_model_loss(xc, enc_o, dec_o, lsd, gsd, lik, 2, 2, num_data=batch)[0])
        ref64 = float(orc.train_model_loss([t.double() for t in xc], enc_6, dec_6, l64, g64, k64, 2, 2, num_data=batch)[0]) \
            if YARDSTICK_AT_SCALE else None
    tr.train_model(x)
    assert math.isfinite(tr.last_loss)
    if ref64 is not None:
        yardstick(f"train_model loss {model}_{width} nc={nc} B={batch}", tr.last_loss, ref, ref64, ratio=1.5, slack=LOSS_BAR)
    assert abs(tr.last_loss - ref) < LOSS_BAR * abs(ref), (tr.last_loss, ref)
    assert math.isfinite(tr.finetune_temporal_encoders(x))


@pytest.mark.parametrize("family", ["vgg", "dcgan"])
def test_full_size_rollout_properties(family):
    """C2 at its full size (B=64, 64x64, 10-in/10-out), where the CPU oracle is too slow to be the checker: size-independent
    properties tie the full-size run to the small runs the oracle validates.
      (a) eval-mode results do not depend on the batch a sample travels in: samples 0..7 of the B=64 rollout equal the
          B=8 rollout of those samples (different tile / split-K choices, same mathematics; GP trigger off because the
          GP couples the samples of a batch by construction);
      (b) hoisting the loop-invariant skip halves (DVG_SKIP_HOIST) does not change the frames;
      (c) the hipGraph replay equals the eager rollout, GP sample included (same eps)."""
    from dvg_amd import fused
    from dvg_amd.rollout import GraphedRollout, sample_rollout
    B, n_past, n_eval = 64, 10, 20
    mods, _ = _build(family, 64, 1, B, 900)
    for m in mods:
        m.to(DEV).eval()
    enc, dec, fp, gp, like = mods
    xs = [params.frames(910 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
    with torch.no_grad():
        full = sample_rollout(enc, dec, fp, gp, like, xs, n_past, n_eval, period=0)
        fp.batch_size = 8
        sub = sample_rollout(enc, dec, fp, gp, like, [t[:8].contiguous() for t in xs], n_past, n_eval, period=0)
        fp.batch_size = B
        for t in range(n_past, n_eval):
            assert rel_err(full[t][:8], sub[t]) < 2e-5, t
        fused.SKIP_HOIST = False
        try:
            plain = sample_rollout(enc, dec, fp, gp, like, xs, n_past, n_eval, period=0)
        finally:
            fused.SKIP_HOIST = True
        for t in range(n_past, n_eval):
            assert rel_err(full[t], plain[t]) < 2e-5, t
        eps = {15: params.normal(930, 90, B).to(DEV)}
        eager = sample_rollout(enc, dec, fp, gp, like, xs, n_past, n_eval, eps_by_step=eps)
        assert all(bool(torch.isfinite(f).all()) for f in eager)
        assert not torch.equal(eager[15], full[15]), "frame 15 is decoded from the GP sample, not from the LSTM output"
    g = GraphedRollout(enc, dec, fp, gp, like, xs, n_past, n_eval)
    a = [f.clone() for f in g()]
    b = [f.clone() for f in g()]
    for t in range(n_past, 15):          # before the trigger step the replay is deterministic and equals eager
        assert rel_err(a[t], eager[t]) < 2e-5 and torch.equal(a[t], b[t]), t
    assert not torch.equal(a[15], b[15]), "fresh GP noise per replay (captured Philox stream)"


def test_condition_once_sample_many_equals_complete_rollouts():
    """generate_frames.make_gifs conditions once per batch and draws every sample with sample_from: each sample must be
    exactly the complete rollout (same eps), and drawing one sample must not disturb the shared conditioning state."""
    from dvg_amd.rollout import condition, sample_from, sample_rollout
    B, n_past, n_eval = 8, 5, 17
    mods, _ = _build("dcgan", 64, 1, B, 950)
    for m in mods:
        m.to(DEV).eval()
    enc, dec, fp, gp, like = mods
    xs = [params.frames(960 + t, B, 1, 64).to(DEV) for t in range(n_eval)]
    eps = [{15: params.normal(970 + s, 90, B).to(DEV)} for s in range(3)]
    with torch.no_grad():
        ref = [sample_rollout(enc, dec, fp, gp, like, xs, n_past, n_eval, eps_by_step=e) for e in eps]
        state = condition(enc, fp, xs, n_past)
        got = [sample_from(state, enc, dec, fp, gp, like, n_past, n_eval, eps_by_step=e) for e in eps]
    for a, b in zip(ref, got):
        assert len(a) == len(b) == n_eval
        for t in range(n_eval):
            assert torch.equal(a[t], b[t]), t
    assert not torch.equal(got[0][16], got[1][16])
