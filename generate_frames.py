#!/usr/bin/env python3
"""generate_frames.py — counterpart of the reference's generate_frames.py on the MI355X kernel library.

Same flags (generate_frames.py:17-41).  Loads `<model_dir>/<dataset>.pth` (falls back to the
`model.pth` that train.py writes — the reference's two scripts disagree on the filename; `--ema`: the averaged
weights of train.py --ema_decay, `<dataset>_ema.pth` else `model_ema.pth`),
takes `opt` from the checkpoint (:44), forces n_eval / n_future / batch_size like :47-49 unless
overridden, and runs either

  * `make_gifs` (:107-217): the posterior rollout (GP fed the LSTM output, predictive MEAN decoded) plus
    `nsample` diverse rollouts where a GP sample replaces the LSTM prediction at steps with i % 15 == 0, or
  * `GPtrigger_gen` (:249-300, `--gp_trigger`): per batch index, a 12-step warm-up that records the norm of
    the GP predictive variance, then a variance-threshold trigger `value > mean + (2+0.01*depth)*std` over a
    12-long sliding window decides per step between a GP sample and the LSTM path.

Results (frames, per-sample SSIM / PSNR, best-of-N index, trigger steps) are saved as tensors, and beside them the
reference's figures: `<log_dir>/gen/sample_lstm_<idx>.gif` (:185-217) and, with `--gp_trigger`,
`<log_dir>/gen/recursive_generation/<index>/heuristic_gp_trigger_<depth>_<n>.png` (plot_rec, :235-245).  The figures are
composed on the device from the rollout tensors (dvg_amd/viz.py, dvg_frame_mosaic): only uint8 pixels are copied to the
host.  `--no_images` writes the tensors only.  `--synthetic_ckpt` builds a randomly initialised checkpoint so the script can
run without a trained model.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import utils  # noqa: E402
from dvg_amd import datasets, mnist, ops, viz  # noqa: E402
from dvg_amd.data import SyntheticMovingMNIST, make_batch_generator, synthetic_video  # noqa: E402
from dvg_amd.rollout import (GraphedSampler, GraphedTrigger, HostTriggerRows, VarianceTrigger, condition, gp_input,  # noqa: E402
                             posterior_from, sample_from, sample_rollout, trigger_body, trigger_log, trigger_warmup)
from dvg_amd.ops import GP_KERNELS  # noqa: E402
from gp_models import GaussianLikelihood, GPRegressionLayer1  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--batch_size', default=50, type=int)
    p.add_argument('--log_dir', default='logs_gp')
    p.add_argument('--model_dir', default='')
    p.add_argument('--name', default='')
    p.add_argument('--data_root', default='./data/kth',
                   help='kth | bair | ucf: the processed dataset tree; frames: train/ and test/ with one directory of frames per clip; smmnist: a directory with the MNIST IDX image files')
    p.add_argument('--seed', default=1, type=int)
    p.add_argument('--image_width', type=int, default=64)
    p.add_argument('--channels', default=1, type=int)
    p.add_argument('--gp_trigger', action='store_true', help='variance-threshold trigger (GPtrigger_gen)')
    p.add_argument('--dataset', default='kth')
    p.add_argument('--n_past', type=int, default=5)
    p.add_argument('--n_future', type=int, default=100)
    p.add_argument('--n_eval', type=int, default=105)
    p.add_argument('--rnn_size', type=int, default=256)
    p.add_argument('--predictor', default='lstm', choices=('lstm', 'gru', 'rnn'),
                   help='--synthetic_ckpt: the frame predictor class to build (a loaded checkpoint runs the class it carries)')
    p.add_argument('--predictor_rnn_layers', type=int, default=2)
    p.add_argument('--gp_kernel', default='rbf', choices=tuple(GP_KERNELS),
                   help='--synthetic_ckpt: the covariance family of the GP layer to build (a loaded checkpoint runs the one its opt names: train.py --gp_kernel)')
    p.add_argument('--z_dim', type=int, default=10)
    p.add_argument('--g_dim', type=int, default=90)
    p.add_argument('--model', default='dcgan')
    p.add_argument('--data_threads', type=int, default=5)
    p.add_argument('--last_frame_skip', action='store_true')
    p.add_argument('--nsample', type=int, default=100)
    p.add_argument('--nbatches', type=int, default=5)
    p.add_argument('--trigger_indices', type=int, default=None, help='GPtrigger_gen: how many batch indices')
    p.add_argument('--synthetic_ckpt', action='store_true')
    p.add_argument('--ema', action='store_true',
                   help='load the averaged weights: <model_dir>/<dataset>_ema.pth, else <model_dir>/model_ema.pth (train.py --ema_decay)')
    p.add_argument('--best', action='store_true',
                   help='load the best checkpoint of train.py --val_every: <model_dir>/model_best.pth, with --ema model_ema_best.pth')
    p.add_argument('--inflight', type=int, default=3,
                   help='make_gifs: samples of a batch drawn at once (one hipGraph + stream each); 0 = eager loop, one at a time')
    p.add_argument('--no_share_prefix', action='store_true',
                   help='make_gifs: run the prediction steps before the first GP trigger step once per SAMPLE, like the reference '
                        'loop (default: once per batch - they are the same for every sample; identical results)')
    p.add_argument('--no_images', action='store_true', help='write the .pt tensors only, no GIF / PNG')
    p.add_argument('--gif_rows', type=int, default=1,
                   help='make_gifs: batch rows to write a GIF for (the reference returns after row 0, generate_frames.py:217)')
    p.add_argument('--metrics', default='skimage', choices=('skimage', 'finn'),
                   help="make_gifs: skimage = utils.eval_seq's 7x7 uniform-window SSIM and PSNR (the reference's script); finn = "
                        "utils.finn_eval_seq's 11x11 Gaussian-window SSIM, PSNR and MSE, the variant KTH / BAIR results are "
                        "published with")
    p.add_argument('--diversity', action='store_true',
                   help='make_gifs: also measure how different the samples are from EACH OTHER (utils.sample_diversity: mean '
                        'pairwise MSE / PSNR between samples and the number of distinct samples, per predicted step); printed per '
                        'batch and saved as `diversity`.  Ignored with --gp_trigger')
    p.add_argument('--gp_report', action='store_true',
                   help='make_gifs: also score the GP trigger\'s predictive on the --nbatches test batches (dvg_amd/gp_score.py: NLPD, '
                        'standardised residuals, coverage, PIT, variance ~ error correlation of the one-step latent forecasts, on '
                        'ground-truth frames and along the posterior rollout); printed at the end, written to <log_dir>/gen/gp_report.json '
                        'and saved as `gp_report`.  Ignored with --gp_trigger')
    p.add_argument('--synthetic_data', action='store_true',
                   help='kth | bair | ucf: synthetic clips of that shape instead of the test split under --data_root; smmnist: '
                        'the in-repo sprites even where --data_root holds MNIST')
    p.add_argument('--trigger', default='period', choices=('period', 'variance'),
                   help="make_gifs: WHEN a sample draws from the GP.  period = at the steps i % 15 == 0, every row of the batch at once "
                        "(the reference's make_gifs); variance = every sequence by itself, at the prediction step where the norm of "
                        "ITS predictive variance exceeds mean + --trigger_coef * std of ITS last --trigger_window values (the "
                        "GPtrigger_gen rule, per row; docs/DESIGN_NOTES_trigger_rows.md).  Not with --gp_trigger")
    p.add_argument('--trigger_window', type=_int_in(1, 64, '--trigger_window'), default=12,
                   help='--trigger variance: values per window, 1..64 (the reference keeps 12)')
    p.add_argument('--trigger_coef', type=float, default=2.01,
                   help="--trigger variance: threshold = mean + coef * std; 2.01 is the reference's 2 + 0.01 * depth at depth 1")
    p.add_argument('--trigger_min_gap', type=_int_in(0, None, '--trigger_min_gap'), default=0,
                   help='--trigger variance: a row that drew at step j may draw again at step i only if i - j > this (0: no limit)')
    datasets.add_resize_arguments(p)      # --resize, --resize_fit: as train.py
    return p


def _int_in(lo, hi, flag):
    def convert(text):
        v = int(text)
        if v < lo or (hi is not None and v > hi):
            raise argparse.ArgumentTypeError('%s must be %s, not %d' % (flag, '>= %d' % lo if hi is None else 'in %d..%d' % (lo, hi), v))
        return v
    return convert


def parse_args(argv=None):
    """build_parser().parse_args plus what argparse cannot say: --trigger variance goes with make_gifs only, and a coefficient
    the window can never exceed gets one warning."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.trigger == 'variance':
        if args.gp_trigger:
            parser.error('--trigger variance is a rule of make_gifs; --gp_trigger runs GPtrigger_gen, which keeps its own')
        if not VarianceTrigger(args.trigger_window, args.trigger_coef, args.trigger_min_gap).can_draw():
            print('WARNING: no sequence will ever draw: ' + (
                'a window of one value has no spread (--trigger_window 1)' if args.trigger_window == 1 else
                '--trigger_coef %g >= sqrt(--trigger_window %d - 1) = %.3f, and no value of a window lies that many population '
                'standard deviations above its mean' % (args.trigger_coef, args.trigger_window, (args.trigger_window - 1) ** 0.5)),
                file=sys.stderr)
    return args


def variance_trigger(opt):
    """The VarianceTrigger the options ask for, None for the period rule."""
    if getattr(opt, 'trigger', 'period') != 'variance':
        return None
    return VarianceTrigger(getattr(opt, 'trigger_window', 12), getattr(opt, 'trigger_coef', 2.01), getattr(opt, 'trigger_min_gap', 0))


def trigger_summary(flags, n_past):
    """(mean, min, max draws per sequence, share of sequences that never drew, mean step of the first draw - nan if none drew)
    over the rows and samples of `flags` (nsample, n_eval, B); torch ops on the device, read once."""
    f = flags[:, n_past:].bool()
    draws = f.sum(1).double()                                                  # (nsample, B)
    drew = draws > 0
    first = n_past + f.int().argmax(1).double()                                # first set step (0 where none: masked below)
    mean_first = (first * drew).sum() / drew.sum() if bool(drew.any()) else torch.tensor(float('nan'))
    return tuple(float(v) for v in (draws.mean(), draws.min(), draws.max(), 1.0 - drew.double().mean(), mean_first))


class Generator:
    def __init__(self, opt, ckpt, device):
        self.opt, self.dev = opt, device
        self.encoder, self.decoder = ckpt['encoder'], ckpt['decoder']
        self.frame_predictor = ckpt['frame_predictor']
        self.likelihood = GaussianLikelihood(batch_size=opt.g_dim)
        # the covariance family the checkpoint was trained with (train.py --gp_kernel, kept in its opt; absent: rbf)
        self.gp_layer = GPRegressionLayer1(opt.g_dim, kernel=getattr(ckpt.get('opt') or opt, 'gp_kernel', 'rbf'))
        self.likelihood.load_state_dict(ckpt['likelihood'])
        self.gp_layer.load_state_dict(ckpt['gp_layer'])
        for m in (self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood):
            m.to(device).eval()
        self.frame_predictor.batch_size = opt.batch_size
        self._sampler, self._sampler_key = None, None
        self.trigger = variance_trigger(opt)      # --trigger variance: rollout.VarianceTrigger; None = the period rule
        # the figures' random sample indices (generate_frames.py:190): a stream of their own, so that writing images draws
        # nothing from the global numpy / torch generators and every saved tensor is what it is without them
        self._viz_rng = np.random.RandomState(opt.seed)
        self._layouts = {}

    def _gp(self, h):
        return self.likelihood(self.gp_layer(gp_input(self.gp_layer, h)))

    @torch.no_grad()
    def make_gifs(self, x, nsample, eps_by_sample=None, diversity=False, host_loop=False, follow=None, guard=0.0):
        """`eps_by_sample[s][i]`: the N(0,1) base sample (D,B) of sample s at trigger step i (parity runs); None = torch RNG.
        diversity: also return utils.sample_diversity of the samples as `diversity` (computed after the sampler has run, from
        the returned tensor; nothing about the rollouts or the other keys changes).
        With --trigger variance the result gains `trigger`: flags (nsample, n_eval, B) int32, values, thresholds and the rule's
        window / coef / min_gap.  host_loop=True (that rule only): the same kernels for everything else, but the variance is read
        back at every step and the decision taken in numpy (rollout.HostTriggerRows) - the cross-check and the timing baseline of
        the device rule; follow (a device run's flags) / guard: a host decision whose margin is inside `guard` takes the device's
        flag and is listed in trigger['followed'] as (sample, step, row)."""
        if host_loop:
            if self.trigger is None:
                raise ValueError("make_gifs: host_loop is the host side of --trigger variance")
            res = self._make_gifs_host(x, nsample, eps_by_sample, follow, guard)
        else:
            res = self._make_gifs(x, nsample, eps_by_sample)
        if diversity:
            res['diversity'] = utils.sample_diversity(res['samples'], self.opt.n_past)
        return res

    def _make_gifs(self, x, nsample, eps_by_sample):
        opt = self.opt
        B, T = x[0].shape[0], opt.n_eval - opt.n_past
        ssim = torch.zeros(B, nsample, T, device=self.dev)
        psnr = torch.zeros(B, nsample, T, device=self.dev)
        finn = getattr(opt, 'metrics', 'skimage') == 'finn'
        mse = torch.zeros(B, nsample, T, device=self.dev) if finn else None
        extra = {'mse': mse, 'metrics': 'finn'} if finn else {}
        all_gen = []
        inflight = getattr(opt, 'inflight', 3)
        trig = self.trigger
        tlog, textra = None, {}
        if trig is not None:
            tlog = {'flags': torch.zeros(nsample, opt.n_eval, B, dtype=torch.int32, device=self.dev),
                    'values': torch.zeros(nsample, opt.n_eval, B, device=self.dev),
                    'thresholds': torch.full((nsample, opt.n_eval, B), float('inf'), device=self.dev)}
            textra = {'trigger': dict(tlog, window=trig.window, coef=trig.coef, min_gap=trig.min_gap)}
        if inflight > 0:
            # One graph per batch for everything the samples share (conditioning, the posterior rollout's prediction steps, the
            # samples' steps before the first GP trigger step) and one per chain for the sample body: rollout.GraphedSampler.
            # Parameter / buffer versions are part of the key: the captured graphs read packed weights and BatchNorm folds of
            # the versions they were captured with, so a weight change (load_state_dict, an optimiser step) re-captures
            share = not getattr(opt, 'no_share_prefix', False)

            def key():
                vers = tuple(t._version for m in (self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood)
                             for t in list(m.parameters()) + list(m.buffers()))
                return (tuple(x[0].shape), len(x), opt.n_past, opt.n_eval, bool(opt.last_frame_skip), inflight, share, finn, vers,
                        ('period',) if trig is None else ('variance',) + trig.key())
            if self._sampler_key != key():
                self._sampler = GraphedSampler(self.encoder, self.decoder, self.frame_predictor, self.gp_layer,
                                               self.likelihood, x, opt.n_past, opt.n_eval, opt.last_frame_skip,
                                               inflight=inflight, share_prefix=None if share else False,
                                               metrics='finn' if finn else 'skimage', trigger=trig)
                # the key AFTER the construction: the sampler's eager warm-up pass may be the GP layer's first call, which
                # initialises its variational parameters in place (gp_models: variational_params_initialized); the graphs are
                # captured after that pass, i.e. with the versions read here
                self._sampler_key = key()
            self._sampler.set_batch(x)
            samples = torch.empty((nsample, opt.n_eval) + tuple(x[0].shape), device=self.dev)
            post = self._sampler.run(nsample, samples, ssim, psnr, eps_by_sample, mse=mse, trigger_log=tlog).clone()
            best = ssim.mean(2).argsort(1)[:, -1]
            return {'posterior': post, 'samples': samples, 'ssim': ssim, 'psnr': psnr, 'best': best, **extra, **textra}
        # everything before the first predicted frame is the same for the posterior rollout and all nsample rollouts of this
        # batch (generate_frames.py:113-121 and :147-162 are the same computation): once per batch
        state = condition(self.encoder, self.frame_predictor, x, opt.n_past, opt.last_frame_skip, decoder=self.decoder)
        post = posterior_from(state, self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood,
                              opt.n_past, opt.n_eval, opt.last_frame_skip)
        tkw = {}
        if trig is not None:     # the conditioning steps' values once per batch; every sample starts from a copy of that state
            base = trig.new_state(B, opt.n_eval, self.dev)
            trig.record_conditioning(base, state['latents'], self.gp_layer, self.likelihood)
            state = dict(state, latents=None)
            tkw = {'trigger': trig, 'trigger_state': trig.new_state(B, opt.n_eval, self.dev)}
        for s in range(nsample):
            if trig is not None:
                trig.copy_state(tkw['trigger_state'], base)
            frames = sample_from(state, self.encoder, self.decoder, self.frame_predictor, self.gp_layer,
                                 self.likelihood, opt.n_past, opt.n_eval, opt.last_frame_skip,
                                 eps_by_step=None if eps_by_sample is None else eps_by_sample[s], **tkw)
            if trig is not None:
                for k in ('flags', 'values', 'thresholds'):
                    tlog[k][s].copy_(tkw['trigger_state'][k])
            if finn:             # utils.finn_eval_seq on device: dvg_eval_frames_finn, all steps in one launch
                m = ops.eval_frames_finn(torch.stack(list(x[opt.n_past:opt.n_eval])), torch.stack(frames[opt.n_past:opt.n_eval]))
                ssim[:, s], psnr[:, s], mse[:, s] = (v.t() for v in m)
            else:
                for t in range(T):   # utils.eval_seq (generate_frames.py:178) on device: dvg_eval_frames
                    ssim[:, s, t], psnr[:, s, t] = ops.eval_frames(x[opt.n_past + t], frames[opt.n_past + t])
            all_gen.append(torch.stack(frames))
        best = ssim.mean(2).argsort(1)[:, -1]   # generate_frames.py:188-189,207: np.argsort(mean_ssim)[-1]
        return {'posterior': torch.stack(post), 'samples': torch.stack(all_gen), 'ssim': ssim, 'psnr': psnr,
                'best': best, **extra, **textra}

    def _score(self, x, frames, s, ssim, psnr, mse):
        """utils.eval_seq / utils.finn_eval_seq of sample s's predicted frames, on the device."""
        opt = self.opt
        if mse is not None:
            m = ops.eval_frames_finn(torch.stack(list(x[opt.n_past:opt.n_eval])), torch.stack(frames[opt.n_past:opt.n_eval]))
            ssim[:, s], psnr[:, s], mse[:, s] = (v.t() for v in m)
        else:
            for t in range(opt.n_eval - opt.n_past):
                ssim[:, s, t], psnr[:, s, t] = ops.eval_frames(x[opt.n_past + t], frames[opt.n_past + t])

    def _make_gifs_host(self, x, nsample, eps_by_sample, follow, guard):
        """make_gifs with --trigger variance as the reference would run it (the pattern of _gp_trigger_gen_host): per step the
        variance goes to the host (`np.linalg.norm(variance.cpu().numpy().transpose(), axis=1)`, generate_frames.py:230, every row),
        numpy slides the windows and decides (:231,288-289), and the flags go back to pick every row's latent."""
        from dvg_amd.rollout import _predict_from
        opt, trig = self.opt, self.trigger
        B, T = x[0].shape[0], opt.n_eval - opt.n_past
        ssim, psnr = torch.zeros(B, nsample, T, device=self.dev), torch.zeros(B, nsample, T, device=self.dev)
        finn = getattr(opt, 'metrics', 'skimage') == 'finn'
        mse = torch.zeros(B, nsample, T, device=self.dev) if finn else None
        state = condition(self.encoder, self.frame_predictor, x, opt.n_past, opt.last_frame_skip, decoder=self.decoder)
        post = posterior_from(state, self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood,
                              opt.n_past, opt.n_eval, opt.last_frame_skip)
        cond_values = [self._variance_norms(self._gp(h)) for h in state['latents']]
        logs = {'flags': np.zeros((nsample, opt.n_eval, B), dtype=np.int32), 'values': np.zeros((nsample, opt.n_eval, B), dtype=np.float32),
                'thresholds': np.full((nsample, opt.n_eval, B), np.inf, dtype=np.float32)}
        followed, all_gen = [], []
        for s in range(nsample):
            host = HostTriggerRows(B, trig.window, trig.coef, trig.min_gap)
            for i, v in enumerate(cond_values, start=1):
                host.step(i, v, False)
                logs['values'][s, i] = v
            near = []

            def latent(i, h, h_pred):
                pred = self._gp(h)
                value = self._variance_norms(pred)
                flags, thr = host.step(i, value, True, None if follow is None else follow[s][i], guard, near)
                logs['values'][s, i], logs['flags'][s, i], logs['thresholds'][s, i] = value, flags, thr
                if i <= trig.window:
                    return h_pred
                z = pred.rsample(None if eps_by_sample is None else eps_by_sample[s][i]).transpose(0, 1)
                return torch.where(torch.from_numpy(flags).to(self.dev).bool().unsqueeze(1), z, h_pred).contiguous()
            frames = _predict_from(state, self.encoder, self.decoder, self.frame_predictor, opt.n_past, opt.n_eval,
                                   opt.last_frame_skip, latent)
            followed += [(s, i, b) for i, b in near]
            self._score(x, frames, s, ssim, psnr, mse)
            all_gen.append(torch.stack(frames))
        best = ssim.mean(2).argsort(1)[:, -1]
        tr = {k: torch.from_numpy(v).to(self.dev) for k, v in logs.items()}
        tr.update(window=trig.window, coef=trig.coef, min_gap=trig.min_gap, followed=followed)
        return {'posterior': torch.stack(post), 'samples': torch.stack(all_gen), 'ssim': ssim, 'psnr': psnr, 'best': best,
                'trigger': tr, **({'mse': mse, 'metrics': 'finn'} if finn else {})}

    def gp_scorer(self):
        """--gp_report: a scorer for this checkpoint's latent size and step counts (dvg_amd/gp_score.py); feed it with
        `score_gp(scorer, x, posterior)` per batch, read it once."""
        from dvg_amd import gp_score
        return gp_score.GPScorer(self.opt.g_dim, gp_score.track_steps(self.opt.n_past, self.opt.n_eval), self.dev)

    def score_gp(self, scorer, x, posterior):
        """One batch: x the ground-truth frames, posterior make_gifs' `posterior` (n_eval, B, C, H, W)."""
        scorer.score(self.encoder, self.gp_layer, self.likelihood, x, posterior, self.opt.n_past, self.opt.n_eval)

    def write_gifs(self, x, res, idx, out_dir, name='lstm', rows=1):
        """generate_frames.py:185-217 on make_gifs' result: `<out_dir>/sample_<name>_<idx + i>.gif` for batch rows i < rows,
        six labelled columns per frame (ground truth, posterior, res['best'][i], three random samples).  One launch composes
        all rows' frames from the tensors where they are; `best` is read on the device.  Returns the paths written."""
        opt = self.opt
        T, B = opt.n_eval, x[0].shape[0]
        H, W = x[0].shape[-2:]
        rows = min(rows, B)
        key = ('gifs', T, opt.n_past, B, H, W, rows)
        if key not in self._layouts:
            self._layouts[key] = viz.make_gifs_layout(T, opt.n_past, B, H, W, rows)
        picks = viz.random_picks(self._viz_rng, rows, 3, res['samples'].shape[0])
        gt = torch.stack(list(x[:T]))
        frames = viz.compose(self._layouts[key], [gt, res['posterior'], res['samples']], best=res['best'], picks=picks).cpu()
        paths = []
        for i in range(rows):
            path = '%s/sample_%s_%d.gif' % (out_dir, name, idx + i)
            if viz.write_gif(path, frames[i * T:(i + 1) * T]):
                paths.append(path)
        return paths

    def write_trigger_pngs(self, res, out_dir, depth=1, frames_generated=0):
        """plot_rec (generate_frames.py:235-245) for every entry of gp_trigger_gen's result: every third frame of the index's
        rollout in one row, `<out_dir>/recursive_generation/<index>/heuristic_gp_trigger_<depth>_<n>.png`."""
        paths = []
        for r in res:
            fr = r['frames'].to(self.dev).unsqueeze(1)                    # (T,1,C,H,W)
            key = ('rec', fr.shape[0]) + tuple(fr.shape[-2:])
            if key not in self._layouts:
                self._layouts[key] = viz.plot_rec_layout(fr.shape[0], fr.shape[-2], fr.shape[-1])
            d = '%s/recursive_generation/%d' % (out_dir, r['index'])
            os.makedirs(d, exist_ok=True)
            paths.append('%s/heuristic_gp_trigger_%d_%d.png' % (d, depth, frames_generated))
            viz.write_png(paths[-1], viz.compose(self._layouts[key], [fr])[0])
        return paths

    @torch.no_grad()
    def _generation(self, x_in, skip):
        h = self.encoder(x_in)[0]
        return self.decoder([self.frame_predictor(h), skip])

    @staticmethod
    def _variance_norms(pred):
        """generate_frames.py:230,275: `np.linalg.norm(final_pred.variance.cpu().detach().numpy().transpose(), axis=1)` -
        per-sample L2 norm over the latent dims of the predictive variance, on the host in float32 like the reference."""
        return np.linalg.norm(pred.variance.cpu().numpy().transpose(), axis=1)

    @torch.no_grad()
    def gp_trigger_gen(self, x, n_index=None, warmup=12, total=105, depth=1, eps_by_step=None, keep_batch=False,
                       indices=None, graph=True, host_loop=False, share_paths=True):
        """generate_frames.py:249-298.  Keeps the reference's bookkeeping verbatim: the warm-up records the
        variance norm of sample `index` (:275) while `var_value` reads sample [3] (:230 - a batch smaller than 4 is an
        IndexError there and an error here); the skip tensors are those of loop steps `i < 5` (:268-269); the rollout is
        autoregressive from x[0]; a triggered step decodes a GP sample and does NOT step the LSTM (:289-292).
        `eps_by_step[i]`: base sample (D,B) for a trigger at step i (parity runs); None = torch RNG.
        indices: the batch indices to run (default range(n_index or B), the reference's `for index in range(batch_size)`).
        Default schedule (rollout.trigger_warmup / trigger_body): the warm-up once per BATCH, one encoder call per step,
        decision and branch select on the device, the main loop a hipGraph (`graph`), logs read back once per index;
        host_loop=True: the reference's own schedule (per index: warm-up, a host round trip and 2-3 encoder calls per step).
        share_paths: the main loop's value is that of sample [3] whatever the index (:230) - only the window's first entries (the
        warm-up norms of the index's own column, :275) differ between indices - so an index whose decisions on an ALREADY
        COMPUTED rollout's values (ops.gp_trigger_replay: the device decision's arithmetic) are that rollout's decisions IS that
        rollout: same frames, no launches.  Applied to rollouts WITHOUT a trigger only: a triggered step draws a GP sample
        from torch's generator, and the reference draws afresh for every index."""
        B = x[0].shape[0]
        if B < 4:
            raise IndexError("GPtrigger_gen reads sample [3] of the batch (generate_frames.py:230): batch_size must be >= 4")
        if indices is None:
            indices = range(B if n_index is None else n_index)
        if host_loop:
            return self._gp_trigger_gen_host(x, indices, warmup, total, depth, eps_by_step, keep_batch)
        mods = (self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood)
        out = []
        if graph:
            def key():     # parameter / buffer versions: the graphs read packed weights and folds of the versions they captured
                return (tuple(x[0].shape), warmup, total, depth,
                        tuple(t._version for m in mods for t in list(m.parameters()) + list(m.buffers())))
            if getattr(self, "_trigger_key", None) != key():
                self._trigger = GraphedTrigger(*mods, x[0], warmup, total, depth)
                self._trigger_key = key()      # AFTER the construction: its eager pass may initialise the GP in place (make_gifs)
            self._trigger.warm(x[0])
            run = lambda index: self._trigger.run(index, eps_by_step)   # noqa: E731
        else:
            dev = x[0].device
            state = trigger_warmup(*mods, x[0], warmup)
            warm_stack = torch.stack(state["frames"])
            eps = torch.zeros(max(1, total - warmup), self.opt.g_dim, B, device=dev)

            def run(index):
                log, ctx = trigger_log(total, dev), state["norms"][:, index].clone()
                if eps_by_step is None:
                    eps.normal_()
                else:
                    for i in range(warmup, total):
                        eps[i - warmup].copy_(eps_by_step[i])
                fr = trigger_body(state, *mods, ctx, 2 + 0.01 * depth, eps, log, warmup, total)
                flags = log["flags"][warmup:].cpu()
                return {"frames": torch.cat([warm_stack, torch.stack(fr)]) if fr else warm_stack,
                        "triggers": [warmup + int(i) for i in torch.nonzero(flags).flatten()],
                        "values": [float(v) for v in torch.cat([state["norms"][:, index], log["values"][warmup:]]).cpu()],
                        "thresholds": [float(v) for v in log["thresholds"][warmup:].cpu()],
                        "values_main": log["values"][warmup:].clone()}
        norms = (self._trigger.state if graph else state)["norms"]
        quiet = []          # computed rollouts without a trigger: (frames (clone), main-loop values on the device)
        self.trigger_rollouts_run = 0
        for index in indices:
            r = None
            if share_paths and total > warmup:
                for fr_q, vm_q in quiet:
                    fl, th = ops.gp_trigger_replay(vm_q, norms[:, index], 2 + 0.01 * depth)
                    if not bool(fl.any()):            # this index decides "no trigger" at every step of that rollout too
                        r = {"frames": fr_q, "triggers": [], "thresholds": [float(v) for v in th.cpu()],
                             "values": [float(v) for v in torch.cat([norms[:, index], vm_q]).cpu()]}
                        break
            if r is None:
                r = run(index)
                self.trigger_rollouts_run += 1
                if share_paths and not r["triggers"] and total > warmup:
                    quiet.append((r["frames"].clone(), r["values_main"]))
            out.append({'index': index, 'frames': r["frames"][:, index].cpu(), 'triggers': r["triggers"],
                        'values': r["values"], 'thresholds': r["thresholds"]})
            if keep_batch:        # parity tests compare the whole batch's frames, not only row `index`
                out[-1]['batch_frames'] = [t.clone() for t in r["frames"]]
        return out

    @torch.no_grad()
    def _gp_trigger_gen_host(self, x, indices, warmup, total, depth, eps_by_step, keep_batch):
        """The reference's schedule, statement for statement (see gp_trigger_gen): kept as the timing baseline of the device
        schedule and as its cross-check (tests/test_gpu_rollouts.py)."""
        out = []
        for index in indices:
            self.frame_predictor.hidden = self.frame_predictor.init_hidden()
            ctx, triggers, gen_seq, values, thresholds = [], [], [], [], []
            x_in, skip = x[0], None
            for i in range(warmup):
                h, sk = self.encoder(x_in)
                if i < 5:
                    skip = sk
                value = self._variance_norms(self._gp(h))[index]
                ctx.append(value)
                values.append(float(value))
                x_in = self._generation(x_in, skip)
                gen_seq.append(x_in)
            ctx = np.array(ctx)
            for i in range(warmup, total):
                h = self.encoder(x_in)[0]
                pred = self._gp(h)
                value = self._variance_norms(pred)[3]
                ctx = np.concatenate([ctx[1:], [value]])
                threshold = np.mean(ctx) + (2 + 0.01 * depth) * np.std(ctx)
                if value > threshold:
                    x_in = self.decoder([pred.rsample(None if eps_by_step is None else eps_by_step[i]).transpose(0, 1),
                                         skip])
                    triggers.append(i)
                else:
                    x_in = self._generation(x_in, skip)
                values.append(float(value))
                thresholds.append(float(threshold))
                gen_seq.append(x_in)
            out.append({'index': index, 'frames': torch.stack(gen_seq)[:, index].cpu(), 'triggers': triggers,
                        'values': values, 'thresholds': thresholds})
            if keep_batch:
                out[-1]['batch_frames'] = gen_seq
        return out


def synthetic_checkpoint(opt):
    import importlib
    import models.lstm as lstm_models
    model = importlib.import_module(f"models.{opt.model}_{opt.image_width}")
    enc, dec = model.encoder(opt.g_dim, opt.channels), model.decoder(opt.g_dim, opt.channels)
    enc.apply(utils.init_weights), dec.apply(utils.init_weights)
    predictor = lstm_models.PREDICTORS[getattr(opt, 'predictor', 'lstm')]
    fp = predictor(opt.g_dim, opt.g_dim, opt.rnn_size, opt.predictor_rnn_layers, opt.batch_size)
    fp.apply(utils.init_weights)
    gp = GPRegressionLayer1(opt.g_dim, kernel=getattr(opt, 'gp_kernel', 'rbf'))
    lik = GaussianLikelihood(batch_size=opt.g_dim)
    return {'encoder': enc, 'decoder': dec, 'frame_predictor': fp, 'likelihood': lik.state_dict(),
            'gp_layer': gp.state_dict(), 'opt': opt}


def data_seed(seed):
    """The seed of the test-split sampler (train.py draws its test batches from the same offset)."""
    return seed + 7919


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic_ckpt:     # (a loaded checkpoint names its own dataset: checked below, once it is read)
        datasets.check_resize(args, 'generate_frames.py')
    assert torch.cuda.is_available(), "generate_frames.py needs a GPU: the DVG hot path has no CPU fallback"
    device = torch.device('cuda', 0)
    if args.synthetic_ckpt:
        ckpt = synthetic_checkpoint(args)
        opt = args
    else:
        path = '%s/%s.pth' % (args.model_dir, args.dataset)
        if args.best:     # the checkpoint train.py --val_every kept (dvg_amd/validate.py); a missing file is a one-line exit
            from dvg_amd.validate import best_checkpoint_path
            path = best_checkpoint_path(args.model_dir, args.ema)
        elif args.ema:    # the averaged weights train.py --ema_decay wrote (same container); a missing file is a one-line exit
            from dvg_amd.ema import checkpoint_path
            path = checkpoint_path(args.model_dir, args.dataset)
        elif not os.path.exists(path):
            path = '%s/model.pth' % args.model_dir
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        opt = ckpt['opt']
        opt.n_eval, opt.n_future, opt.batch_size = args.n_eval, args.n_future, args.batch_size
        opt.log_dir = args.log_dir
        opt.inflight = args.inflight
        opt.metrics = args.metrics
        opt.trigger, opt.trigger_window = args.trigger, args.trigger_window
        opt.trigger_coef, opt.trigger_min_gap = args.trigger_coef, args.trigger_min_gap
    os.makedirs('%s/gen/' % opt.log_dir, exist_ok=True)
    print("Random Seed: ", opt.seed)
    random.seed(opt.seed)
    torch.manual_seed(opt.seed)
    torch.cuda.manual_seed_all(opt.seed)
    gen = Generator(opt, ckpt, device)
    dataset = getattr(opt, 'dataset', 'smmnist')
    datasets.check_resize(argparse.Namespace(resize=getattr(args, 'resize', 'none'), resize_fit=getattr(args, 'resize_fit', 'crop'),
                                             dataset=dataset, synthetic_data=args.synthetic_data), 'generate_frames.py')
    real_digits = dataset == 'smmnist' and not args.synthetic_data and mnist.find_tree(args.data_root, False) is not None
    if (dataset != 'smmnist' and not args.synthetic_data) or real_digits:
        # the test split under --data_root (the command line's, not the checkpoint's), as generate_frames.py:89-104; smmnist
        # takes this branch when the MNIST image files are there (dvg_amd/mnist.py)
        opt.data_root, opt.data_threads, opt.synthetic_data = args.data_root, args.data_threads, False
        opt.resize, opt.resize_fit = datasets.resize_spec(args) or ('none', 'crop')      # the command line's, like --data_root
        opt.num_digits = getattr(opt, 'num_digits', 2)
        opt.local_batch, opt.rank = opt.batch_size, 0
        test_gen = make_batch_generator(opt, opt.n_eval, data_seed(opt.seed), device, train=False)
        batches = (next(test_gen)() for _ in range(args.nbatches))
    else:
        print("WARNING: synthetic data - %s; --data_root is ignored" %
              ("Moving-MNIST trajectories over synthetic sprites (not MNIST digits)" if dataset == 'smmnist'
               else f"random textured clips shaped like {dataset}"), file=sys.stderr)
        if dataset == 'smmnist':
            ds = SyntheticMovingMNIST(seq_len=opt.n_eval, image_size=opt.image_width, seed=opt.seed + 7919)
            seqs = (ds.batch(opt.batch_size) for _ in range(args.nbatches))
        else:
            seqs = (synthetic_video(opt.batch_size, opt.n_eval, opt.channels, opt.image_width, seed=opt.seed + k)
                    for k in range(args.nbatches))
        batches = (utils.normalize_data(opt, torch.cuda.FloatTensor, seq)[0] for seq in seqs)
    if args.diversity and args.gp_trigger:
        print("WARNING: --diversity scores make_gifs' samples; ignored with --gp_trigger", file=sys.stderr)
    if args.gp_report and args.gp_trigger:
        print("WARNING: --gp_report scores make_gifs' batches; ignored with --gp_trigger", file=sys.stderr)
    scorer = gen.gp_scorer() if args.gp_report and not args.gp_trigger else None
    written = []
    for i, test_x in enumerate(batches):
        if args.gp_trigger:
            res = gen.gp_trigger_gen(test_x, args.trigger_indices, total=opt.n_eval)
            torch.save(res, '%s/gen/gp_trigger_%d.pt' % (opt.log_dir, i))
            print('batch %d: trigger steps of index 0: %s' % (i, res[0]['triggers']))
            if not args.no_images:
                gen.write_trigger_pngs(res, '%s/gen' % opt.log_dir)
        else:
            res = gen.make_gifs(test_x, args.nsample, diversity=args.diversity)
            if scorer is not None:      # accumulated on the device over the batches; read once, after the last
                gen.score_gp(scorer, test_x, res['posterior'])
            saved = {'posterior': res['posterior'][:, 0].cpu(), 'best': res['best'].cpu(), 'psnr': res['psnr'].cpu(),
                     'ssim': res['ssim'].cpu(),
                     'best_sample_0': res['samples'][int(res['best'][0]), :, 0].cpu()}
            if 'mse' in res:
                saved.update(mse=res['mse'].cpu(), metrics=res['metrics'])
            if 'diversity' in res:
                saved['diversity'] = {k: v.cpu() for k, v in res['diversity'].items()}
            if 'trigger' in res:
                saved['trigger'] = {k: v.cpu() if torch.is_tensor(v) else v for k, v in res['trigger'].items()}
            torch.save(saved, '%s/gen/sample_lstm_%d.pt' % (opt.log_dir, i))
            scorer is None or written.append(('%s/gen/sample_lstm_%d.pt' % (opt.log_dir, i), saved))
            sel = res['best'].view(-1, 1, 1).expand(-1, 1, res['ssim'].shape[2])
            if 'mse' in res:
                print('batch %d: best-of-%d by mean Finn SSIM (11x11 Gaussian window): SSIM %.4f, PSNR %.3f dB, MSE %.3e' % (
                    i, args.nsample, float(res['ssim'].gather(1, sel).mean()), float(res['psnr'].gather(1, sel).mean()),
                    float(res['mse'].gather(1, sel).mean())))
            else:
                print('batch %d: best-of-%d by mean SSIM: SSIM %.4f, PSNR %.3f dB' % (
                    i, args.nsample, float(res['ssim'].gather(1, sel).mean()), float(res['psnr'].gather(1, sel).mean())))
            if 'diversity' in res:
                dv = res['diversity']
                print('batch %d: between the %d samples: pairwise MSE %.3e, PSNR %.3f dB over the predicted steps; distinct '
                      'samples at the last step %.1f/%d' % (i, args.nsample, float(dv['pair_mse'].mean()),
                                                            float(10.0 * torch.log10(1.0 / dv['pair_mse'].mean())),
                                                            float(dv['distinct'][:, -1].double().mean()), args.nsample))
            if 'trigger' in res:
                tr = res['trigger']
                mean, lo, hi, never, first = trigger_summary(tr['flags'], opt.n_past)
                print('batch %d: variance trigger (window %d, coef %g, min gap %d): draws per sequence mean %.2f min %d max %d; %.1f %% '
                      'of the sequences never drew; mean step of the first draw %.1f' % (
                          i, tr['window'], tr['coef'], tr['min_gap'], mean, lo, hi, 100.0 * never, first))
            if not args.no_images:
                gen.write_gifs(test_x, res, i, '%s/gen' % opt.log_dir, rows=args.gif_rows)
    if scorer is not None and written:
        from dvg_amd import gp_score
        gen.gp_report = scorer.read()
        for tag in gp_score.TRACKS:
            pooled = gen.gp_report[tag]['pooled']
            print('gp %s (%d entries, %d skipped): nlpd %.4f rmse %.5f mean var %.5f z mean %.3f z std %.3f cover 68/95 %.3f / %.3f '
                  'pit err %.3f var~err corr %.3f smse %.4f' % (
                      tag, pooled['taken'], pooled['skipped'], *(gp_score._num(pooled[k]) for k in (
                          'nlpd', 'rmse', 'mean_var', 'z_mean', 'z_std', 'cover68', 'cover95', 'pit_err', 'var_err_corr', 'smse'))))
            print(gp_score.curves(tag, gen.gp_report[tag]))
        gp_score.write_report(gen.gp_report, '%s/gen' % opt.log_dir)
        for path, saved in written:     # the saved tensors gain `gp_report`: the report of all the batches, known only now
            torch.save(dict(saved, gp_report=gen.gp_report), path)
    return gen


if __name__ == '__main__':
    main()
