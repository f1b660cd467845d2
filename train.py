#!/usr/bin/env python3
"""train.py — counterpart of the reference's train.py on the MI355X kernel library.

Same flags (train.py:17-46) and the same three step closures (`train_model` :200-248,
`train_frame_predictor` :175-198, `train_GP_Frame_predictor` :146-172), loss weights (:239), optimisers
(:95-106, lr hard-coded 0.002 like the reference; `--lr/--beta1/--z_dim/--name` stay accepted
and unused - `--lr` except under `--lr_schedule` or an `--optimizer` other than adam), scheduler-before-epoch order (:347), log line (:368) and checkpoint dict (:380-388).
This file is the command line: flags, `options`, the epoch loop.  The closures and the iteration are `Trainer`, dvg_amd/trainer.py.

Consciously fixed (each was unrunnable in the reference — SURVEY.md §5 quirks):
  * the model family follows `--model` / `--image_width` instead of a hard-coded dcgan_64 (:75);
  * `h.view(90, 50, 1)` (:164) uses `(g_dim, batch_size, 1)`;
  * `--dataset smmnist` works (`--num_digits`), batches may be `x` or `(x, y)`;
  * no `torch.cuda.empty_cache()` per timestep (:166,191,235);
  * `--ft` / flags are real booleans (`--no_ft`).
Reference behaviour that is KEPT although it looks like a bug, with a switch (each has a test showing both modes):
  * `Trainer.reference_gp_grad_leak = True`: train_model (:200-245) zeroes the encoder / decoder / LSTM gradients but
    not the GP optimiser's, so the full-scale ELBO gradients that the previous iteration's train_GP_Frame_predictor
    left in `.grad` (:170-171) are still there when train_model's `optimizer.step()` (:245) runs, on top of the
    1e-4-weighted ones of :239.  False zeroes them first.
Added: data parallelism — launch with `python -m torch.distributed.run --nproc-per-node N train.py ...`;
`--batch_size` is the GLOBAL batch, split evenly over the ranks (the ELBO's `num_data` is the global batch as well, so
the KL weight does not change with the number of GPUs); every parameter's `.grad` is a view of one flat arena
(dvg_amd/optim.py) whose ranges are averaged in place over RCCL, the decoder-side range while the encoder phase of the
backward pass is still running (dvg_amd/parallel.py); BatchNorm statistics are per replica.
Datasets: `kth | bair | ucf` read the reference's processed tree under `--data_root` (dvg_amd/datasets.py: decoded once into
a device frame pool, batches gathered by dvg_clip_gather_u8) - or, with `--synthetic_data`, train on random textured clips of
that shape; `smmnist` = the reference's Moving-MNIST over the MNIST IDX image files under `--data_root` (dvg_amd/mnist.py: no
torchvision, no download; scaled to 32x32 once on the device, a batch is one dvg_moving_mnist_compose_u8 launch) - or, without
those files or with `--synthetic_data`, seeded Moving-MNIST trajectories with in-repo sprites, announced by a warning.
`--resume PATH` continues a run exactly from the `train_state.pth` written beside `model.pth` (the reference's "load the trained
model" section, :86, is empty and `--model_dir` is never read: both kept); dvg_amd/train_state.py, docs/DESIGN_NOTES_resume.md.
`--ema_decay D` keeps an exponential moving average of all weights on the device, one launch per iteration inside the captured
graph, and writes `model_ema.pth` beside `model.pth` (dvg_amd/ema.py, docs/DESIGN_NOTES_ema.md).
`--augment LIST` (kth | bair | ucf, train split): flip / reverse / shift / jitter per clip, applied inside the gather
(dvg_clip_gather_aug_u8; dvg_amd/datasets.py ClipAugmenter, docs/DESIGN_NOTES_augment.md).
`--dataset frames --resize FILTER [--resize_fit crop|stretch]`: a folder of clips, <root>/{train,test}/.../<clip>/<frame>.png|jpg, frames
of any size; `--resize` scales every frame that is not image_width x image_width on the device while the frame pool is built, bit-equal
to Pillow's Image.resize (dvg_resample_u8; dvg_amd/resample.py, docs/DESIGN_NOTES_frames.md).  It applies to kth | bair | ucf trees too.
`--val_every N` scores a fixed set of held-out clips every N epochs on rank 0 (eval-mode rollouts, Finn metrics, dvg_val_accumulate),
logs them to `val_log.jsonl` and keeps `model_best.pth` (dvg_amd/validate.py, docs/DESIGN_NOTES_validation.md).
`--val_gp` adds the held-out scores of the GP trigger's predictive to every validation: NLPD, standardised residuals, coverage, PIT,
variance ~ error correlation of the one-step latent forecasts (dvg_gp_score; dvg_amd/gp_score.py, docs/DESIGN_NOTES_gp_score.md).
`--lr_schedule KIND` makes `--lr` the base rate of all four optimisers and moves it every iteration by a device-side multiplier:
warm-up, then constant | linear | cosine | step; one launch per iteration (dvg_amd/lr_schedule.py, docs/DESIGN_NOTES_lr_schedule.md).
`--frame_loss l1|charbonnier`, `--gdl_weight G`, `--ssim_weight W`: another pixel penalty / the gradient-difference loss / 1 - SSIM in the frame terms
(dvg_amd/frame_loss.py).
`--optimizer adam|adamw|sgd|rmsprop`, `--weight_decay W`, `--momentum M`, `--nesterov`, `--rmsprop_alpha A`: the update rule of all four
optimisers (the reference accepts --optimizer and builds Adam whatever it says, :95-104) and a decay of the weight matrices of the
encoder, decoder and frame predictor, one dvg_optim_step launch per group (dvg_amd/optim.py, docs/DESIGN_NOTES_optimizers.md).
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from dvg_amd import datasets, ema as weight_ema, frame_loss, lr_schedule, optim, parallel, train_state, validate  # noqa: E402
from dvg_amd.data import make_batch_generator  # noqa: E402
# the Trainer (dvg_amd/trainer.py), the hipGraph replay of its iteration and the batch prefetcher (dvg_amd/train_graphs.py),
# re-exported for `train.<name>`
from dvg_amd.ops import GP_KERNELS  # noqa: E402
from dvg_amd.optim import guard_options  # noqa: E402,F401
from dvg_amd.train_graphs import BatchPrefetcher, GraphedIteration, SegmentedIteration  # noqa: E402,F401
from dvg_amd.trainer import Trainer  # noqa: E402,F401


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--lr', default=0.002, type=float, help='unused, as in the reference; under --lr_schedule or an --optimizer other than adam: the base rate of all four optimisers')
    p.add_argument('--beta1', default=0.9, type=float)
    p.add_argument('--batch_size', default=50, type=int, help='GLOBAL batch size')
    p.add_argument('--log_dir', default='logs')
    p.add_argument('--model_dir', default='', help='accepted and unused, as in the reference; to continue a run: --resume')
    p.add_argument('--resume', default='', metavar='PATH',
                   help='continue exactly from a train_state.pth (or the directory that holds one; written beside model.pth) at '
                        'the saved epoch; the other options must be those of the run that saved it (docs/DESIGN_NOTES_resume.md)')
    p.add_argument('--name', default='')
    p.add_argument('--output_path', default='.')
    p.add_argument('--data_root', default='path/to/data/',
                   help='kth | bair | ucf: the root of the processed dataset tree; frames: a directory with train/ and test/, '
                        'below them one directory of .png / .jpg frames per clip; smmnist: a directory holding the MNIST IDX '
                        'image files (<root>/MNIST/raw, <root>/raw or <root>, raw or .gz)')
    p.add_argument('--niter', type=int, default=601)
    p.add_argument('--seed', default=1, type=int)
    p.add_argument('--epoch_size', type=int, default=300)
    p.add_argument('--image_width', type=int, default=64)
    p.add_argument('--channels', default=1, type=int)
    p.add_argument('--dataset', default='smmnist')
    p.add_argument('--num_digits', type=int, default=2)
    p.add_argument('--n_past', type=int, default=5)
    p.add_argument('--no_ft', action='store_true', help='disable the temporal fine-tuning closures')
    p.add_argument('--n_future', type=int, default=10)
    p.add_argument('--n_eval', type=int, default=15)
    p.add_argument('--rnn_size', type=int, default=256)
    p.add_argument('--predictor', default='lstm', choices=('lstm', 'gru', 'rnn'),
                   help='the frame predictor\'s cell: the reference\'s models.lstm.lstm (default), .gru or .rnn; gru trains in the '
                        'sequence form like lstm, rnn step by step.  Part of the --resume fingerprint when it is not lstm')
    p.add_argument('--predictor_rnn_layers', type=int, default=2)
    # (no attribute without the flag: the options of such a run - printed, pickled into its checkpoints - are what they always were)
    p.add_argument('--gp_kernel', default=argparse.SUPPRESS, choices=tuple(GP_KERNELS),
                   help='the covariance of the GP trigger: the reference\'s ScaleKernel(RBFKernel) (rbf, also what no flag means) or '
                        'ScaleKernel(MaternKernel(nu)) with nu = 1/2, 3/2, 5/2 - same parameters, same checkpoint keys; stored in '
                        'the checkpoint\'s opt, which generate_frames.py reads.  Part of the --resume fingerprint when it is not rbf')
    p.add_argument('--z_dim', type=int, default=10)
    p.add_argument('--g_dim', type=int, default=90)
    p.add_argument('--model', default='dcgan', help='dcgan | vgg')
    p.add_argument('--data_threads', type=int, default=5)
    p.add_argument('--last_frame_skip', action='store_true')
    p.add_argument('--save_every', type=int, default=4)
    p.add_argument('--no_save', action='store_true')
    p.add_argument('--no_images', action='store_true', help='do not write sample_<epoch>.png / .gif beside the tensors')
    p.add_argument('--hip_graph', action='store_true',
                   help='(the default) replay each training iteration as one hipGraph (GraphedIteration; same losses and '
                        'parameters as the eager loop, tested; 1.5-2.7x the train frames/s); with more than one rank: as a '
                        'chain of hipGraphs cut at the gradient all-reduces, which stay eager (SegmentedIteration)')
    p.add_argument('--no_hip_graph', action='store_true', help='eager launches for every iteration')
    p.add_argument('--print_param_checksum', action='store_true',
                   help='print a checksum of all parameters per rank at the end (multi-rank tests: every rank must agree)')
    p.add_argument('--sync_bn', action='store_true',
                   help='several ranks: BatchNorm statistics (and their backward sums) over the GLOBAL batch - one all-reduce of '
                        '2 x C floats per BatchNorm call and direction - i.e. the reference\'s single-process semantics: N ranks x '
                        'B/N clips then train exactly like one process on B clips (default: per-replica statistics, as '
                        'DistributedDataParallel).  The collectives cannot be captured in a hipGraph: iterations run eager.')
    p.add_argument('--synthetic_data', action='store_true',
                   help='kth | bair | ucf: train on synthetic clips of that shape instead of reading --data_root; smmnist: '
                        'the in-repo sprites even where --data_root holds MNIST')
    for mod in (optim, weight_ema, datasets, validate, lr_schedule, frame_loss):   # guard flags, --ema_decay, --augment, --val_*, --lr_*, --frame_loss
        mod.add_arguments(p)
    return p


def options(argv=None, *, rank=0, world=1, local_batch=None):
    """The parsed command line plus the fields derived from it that a Trainer reads: `ft`, `rank`, `world` and `local_batch`
    (this rank's share of the global --batch_size unless given)."""
    opt = build_parser().parse_args(argv)
    opt.ft = not opt.no_ft
    opt.rank, opt.world = rank, world
    opt.local_batch = parallel.shard_batch(opt.batch_size, world) if local_batch is None else local_batch
    optim.optimizer_options(opt)   # --optimizer and its companions: refused here, before anything is built
    getattr(opt, "val_gp", False) and validate.options(opt)   # --val_gp without --val_every: likewise
    return opt


def main(argv=None):
    rank, world, local = parallel.init_distributed()
    opt = options(argv, rank=rank, world=world)
    opt.augment = datasets.check_augment(opt)   # --augment: parsed and refused before anything is built
    datasets.check_resize(opt)                  # --resize: likewise
    if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
        # the latent path of an eager iteration runs on a second stream on purpose (autograd.JOIN_STREAMS joins them)
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    state = train_state.open_resume(opt)    # --resume: read and checked against the options before anything is built
    if rank == 0:
        print("Random Seed: ", opt.seed)
        if opt.augment:
            print(f"augment: {opt.augment} (train split only)")
    random.seed(opt.seed + rank)
    np.random.seed(opt.seed + rank)
    torch.manual_seed(opt.seed)          # identical init on every rank (also broadcast below)
    assert torch.cuda.is_available(), "train.py needs a GPU: the DVG hot path has no CPU fallback"
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    torch.cuda.manual_seed_all(opt.seed)
    rank == 0 and print(opt)
    tr = Trainer(opt, device)
    torch.manual_seed(opt.seed + 1000 * rank)   # from here on: per-rank randomness (GP samples)
    train_gen = BatchPrefetcher(make_batch_generator(opt, opt.n_past + opt.n_future, opt.seed + 17 * rank, device))
    test_gen = make_batch_generator(opt, opt.n_eval, opt.seed + 7919 + 17 * rank, device, train=False)
    # One rank: the iteration as one hipGraph.  Several ranks: a chain of hipGraphs cut at the gradient all-reduces, which
    # stay eager (SegmentedIteration).  Capturing the RCCL collectives inside ONE graph instead is NOT safe
    # on this stack: the c10d watchdog thread may query a collective's event while it is "recorded in a capturing stream"
    # (hipErrorCapturedEvent) and terminate the process (1 of 5 runs with a one-rank RCCL group).
    if opt.no_hip_graph or tr.sync_bn:
        step = tr.iteration
    elif world == 1:
        step = GraphedIteration(tr)
    else:
        step = SegmentedIteration(tr)
    first_epoch = train_state.resume(tr, state, train_gen, test_gen)
    for epoch in range(first_epoch, opt.niter):
        tr.train_mode()
        tr.scheduler.step()   # before the epoch, as train.py:347
        epoch_mse = 0.0
        t0, indices = time.time(), 0.0
        for i in range(opt.epoch_size):
            x = next(train_gen)()
            mse_ctrl, indices, temp_loss = step(x)
            epoch_mse += mse_ctrl + temp_loss
        torch.cuda.synchronize()
        if rank == 0:
            fps = opt.batch_size * (opt.n_past + opt.n_future - 1) * opt.epoch_size / (time.time() - t0)
            print('[%02d] mse loss: %.5f (%d) %.5f' % (epoch, epoch_mse / opt.epoch_size,
                                                       epoch * opt.epoch_size * opt.batch_size, indices))
            print('     train frames/s: %.1f' % fps)
        for part in (tr.guard, tr.ema, tr.lr_schedule, tr.frame_terms, tr.optim_report, tr.gp_report):   # one read of each one's device counters: per epoch, outside the iterations
            line = part is not None and part.epoch_line()   # every rank reads its own (the same bits everywhere; frame loss: its shard's means), rank 0 prints
            line and rank == 0 and print(line)
        if epoch % opt.save_every == 0:
            tr.frame_predictor.eval()
            tr.gp_layer.eval()
            tr.likelihood.eval()   # encoder / decoder stay in train mode, as train.py:372-374
            test_x = next(test_gen)()
            gen, best = tr.plot(test_x, epoch)
            if rank == 0 and not opt.no_save:
                os.makedirs(opt.output_path, exist_ok=True)
                torch.save({'gen': gen[:, :, :min(opt.local_batch, 10)].cpu(), 'best': best.cpu()},
                           '%s/sample_%d.pt' % (opt.output_path, epoch))
                tr.save('%s/model.pth' % opt.output_path)
                tr.ema is None or tr.ema.save(tr, '%s/%s' % (opt.output_path, weight_ema.FILE))   # model_ema.pth
                opt.no_images or tr.write_plot(test_x, gen, best, epoch, opt.output_path)   # sample_<epoch>.png / .gif
        validate.after_epoch(tr, epoch)   # --val_every (rank 0): after the checkpoint, before the state that carries its history
        if epoch % opt.save_every == 0 and not opt.no_save:   # after all of this epoch that draws random numbers; rank 0: the shared part too
            train_state.write(tr.state_dict(epoch + 1, train_gen, test_gen, shared=rank == 0), opt.output_path, rank, world)
        epoch % 10 == 0 and rank == 0 and print('log dir: %s' % opt.log_dir)
    if opt.print_param_checksum:   # tests: every rank must end with the same parameters
        weight_ema.print_checksums(tr, rank)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return tr


if __name__ == '__main__':
    main()
