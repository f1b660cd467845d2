"""The Trainer: the module-level state of the reference's train.py as an object, its three step closures and the iteration
that strings them together.  train.py keeps the command line (flags, the epoch loop, the log lines and checkpoints) and
re-exports `Trainer`; how an iteration is replayed as hipGraphs is dvg_amd/train_graphs.py.  `train.py:NNN` in the comments
below are line numbers of the reference's train.py."""
import importlib
import os

import torch
import torch.nn as nn

from . import _derived, ema as weight_ema, frame_loss, fused, lr_schedule, parallel, train_state, validate, viz
from .models import lstm as lstm_models
from .models.gp_models import GaussianLikelihood, GPRegressionLayer1, VariationalELBO
from .optim import FlatArena, OptimizerReport, guarded_step, make_guard, make_optimizer, optimizer_options, zero_grads
from .rollout import frames_as_batch, gp_input
from .utils import init_weights


class GPKernelReport:
    """train.py's epoch line of --gp_kernel (None without the flag or with rbf: no line, no read)."""

    def __init__(self, gp_layer):
        self.gp_layer = gp_layer

    @torch.no_grad()
    def epoch_line(self) -> str:
        s, ell, _ = self.gp_layer.hypers()
        ell_mean, s_mean = torch.stack([ell.mean(), s.mean()]).tolist()      # one read of the device, once per epoch
        return '     gp kernel: %s  mean lengthscale %.4f  mean outputscale %.4f' % (self.gp_layer.kernel, ell_mean, s_mean)


class Trainer:
    """The module-level state of the reference script, as an object (so tests can drive single steps)."""

    def __init__(self, opt, device):
        self.opt, self.dev = opt, device
        self.rank, self.world = opt.rank, opt.world
        model = importlib.import_module(f"dvg_amd.models.{opt.model}_{opt.image_width}")
        self.encoder = model.encoder(opt.g_dim, opt.channels)
        self.decoder = model.decoder(opt.g_dim, opt.channels)
        self.encoder.apply(init_weights)
        self.decoder.apply(init_weights)
        # --predictor: the reference's lstm (the default), gru or rnn (lstm.py:42-136)
        predictor = lstm_models.PREDICTORS[getattr(opt, "predictor", "lstm")]
        self.frame_predictor = predictor(opt.g_dim, opt.g_dim, opt.rnn_size, opt.predictor_rnn_layers, opt.local_batch)
        self.frame_predictor.apply(init_weights)
        # --gp_kernel: the GP's covariance family, the reference's rbf (the default) or a Matern member
        self.gp_layer = GPRegressionLayer1(num_dims=opt.g_dim, kernel=getattr(opt, "gp_kernel", "rbf"))
        self.likelihood = GaussianLikelihood(batch_size=opt.g_dim)
        self.modules = [self.encoder, self.decoder, self.frame_predictor, self.gp_layer, self.likelihood]
        for m in self.modules:
            m.to(device)
        # True = the reference's behaviour: train_model does not zero the GP optimiser's gradients (see train.py's docstring)
        self.reference_gp_grad_leak = True
        # True = backward in two phases (decoder / LSTM / GP side, then the encoder) so that the all-reduce of the first
        # phase's gradients overlaps the second phase; needs share_encoder_passes
        self.staged_backward = True
        # True = back-propagate into the encoder in the two fine-tuning closures like the reference does (and then
        # discards); kept only so that tests can show both ways give the same updates
        self.finetune_encoder_grad = False
        # False = encode every middle frame twice per closure like the reference does (tests compare both ways)
        self.share_encoder_passes = True
        # True = the three decoder calls of a time step compute the skip half of each concat conv once (forward + backward)
        self.share_skip_halves = True
        # True = the GP fine-tuning closure reuses the encodings of the LSTM fine-tuning closure that precedes it
        self.share_closure_encodings = True
        # True = the encoder calls of a closure run as ONE pass over all frames with per-frame ("grouped") BatchNorm
        # statistics (needs share_encoder_passes); DVG_TIME_BATCH=0: one pass per frame
        self.time_batched = os.environ.get("DVG_TIME_BATCH", "2") != "0"
        # True (with time_batched) = train_model's 3 S decoder calls as one decoder pass with shared skip blocks
        # (_train_model_batched); DVG_TIME_BATCH=1: encoder only
        self.time_batched_decoder = os.environ.get("DVG_TIME_BATCH", "2") not in ("0", "1")
        # True (with time_batched) = the LSTM of a teacher-forced closure over the whole sequence at once: one GEMM per
        # non-recurrent product over all S x B rows, one launch per step and layer for the recurrence (models.lstm.
        # forward_sequence); lstm_sequence = False: one module call per step (an environment switch until r06)
        self.lstm_sequence = True
        # True = train_model's latent path (LSTM, GP, latent losses) on a second stream, concurrent with the decoder calls
        self.latent_stream = True
        # True = the closures' losses and their gradients by dvg_frame_losses / dvg_mse_sum_grad, backward seeded with them
        # (no scalar autograd graph of torch ops); False: the torch composition (tests compare the two)
        self.fused_losses = True
        self._loss_w = {}
        self._side_stream = None
        self._iters = 0            # iterations since reset_allreduce_stats (allreduce_stats divides by it)
        self.last_loss = None      # train_model's total loss of the last iteration, as a float
        self._ft_cache = None      # the LSTM fine-tuning closure's encodings, for the GP closure that follows it
        self._segmenter = None     # the SegmentedIteration that is capturing: _ar cuts its graph instead of reducing
        self._ar_pending = {}      # started, unfinished gradient all-reduces by key
        self._plot_writer = None   # viz.PlotWriter, made by the first write_plot
        self.state_loads = 0       # load_state_dict calls: GraphedIteration re-captures when it moves
        # optim.Adam(lr=0.002) x4 (train.py:95-104) as one fused HIP launch per parameter group.  All groups live in ONE
        # flat arena in the order [GP | likelihood | LSTM | decoder | encoder]: parameters, gradients (p.grad are views)
        # and both moments; the data-parallel all-reduce works on ranges of arena.g in place.
        # --optimizer / --weight_decay: another rule (dvg_optim_step) and the decay masks; None = FusedAdam as ever.  HIP only,
        # like the models themselves: no CPU fallback on the product path
        spec = optimizer_options(opt)
        allp = [p for m in self.modules for p in m.parameters()]
        self.arena = FlatArena(FlatArena.size_for(allp), device)
        lr = lr_schedule.base_rate(opt)   # 0.002, as the reference; --lr under --lr_schedule or a rule other than adam
        self.optimizer = make_optimizer(spec, "gp", [{'params': self.gp_layer.parameters()},
                                                     {'params': self.likelihood.parameters()}], lr, self.arena)
        self.frame_predictor_optimizer = make_optimizer(spec, "frame_predictor", self.frame_predictor.parameters(), lr, self.arena)
        self.decoder_optimizer = make_optimizer(spec, "decoder", self.decoder.parameters(), lr, self.arena)
        self.encoder_optimizer = make_optimizer(spec, "encoder", self.encoder.parameters(), lr, self.arena)
        # the epoch line of the new flags; None = nothing exists
        self.optim_report = spec and OptimizerReport(spec, self.optimizers(), self.arena.p.numel())
        self.gp_report = GPKernelReport(self.gp_layer) if self.gp_layer.kernel != "rbf" else None
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=[3, 5], gamma=0.1)
        # num_data = the GLOBAL batch (train.py:112 passes opt.batch_size): each rank's loss is ll_r/B_local - KL/num_data and
        # the ranks are averaged, which gives the reference's ll/B - KL/B at the same global batch for any number of ranks
        self.mll = VariationalELBO(self.likelihood, self.gp_layer, num_data=opt.batch_size, combine_terms=True)
        self.mse_criterion = nn.MSELoss()
        self.mse_latent_criterion = nn.MSELoss()
        # every replica starts from rank 0's values: ONE broadcast of the parameter arena (all parameters are views of it by
        # now) + one packed broadcast per buffer dtype, instead of ~200 per-tensor broadcasts
        self.broadcast_collectives = parallel.broadcast_parameters(self.modules, arena_p=self.arena.p)
        # --sync_bn: BatchNorm over the global batch (fused.set_sync_bn).  Its small collectives get their OWN process group
        # (own RCCL communicator and stream): they must not queue behind the gradient ranges that are in flight while the
        # encoder phase of the backward pass - which issues them - is still running
        self.sync_bn = False
        if getattr(opt, 'sync_bn', False) and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            fused.set_sync_bn(torch.distributed, torch.distributed.new_group())
            self.sync_bn = True
        self.reducer = parallel.ArenaReducer(self.arena.g)
        self.rng_gp = (self.optimizer.flat_range(0)[0], self.optimizer.flat_range(1)[1])
        self.rng_fp = self.frame_predictor_optimizer.flat_range(0)
        self.rng_dec = self.decoder_optimizer.flat_range(0)
        self.rng_enc = self.encoder_optimizer.flat_range(0)
        assert self.rng_gp[1] == self.rng_fp[0] and self.rng_fp[1] == self.rng_dec[0] and self.rng_dec[1] == self.rng_enc[0]
        # --clip_grad_norm / --skip_nonfinite: one device-side verdict per step site (_step); None = every site steps as ever
        self.guard = make_guard(opt, device, self.optimizers())
        # --ema_decay: an averaged copy of arena.p (after the broadcast above), moved once per iteration; None = nothing exists
        self.ema = weight_ema.make_average(opt, self.arena)
        # --lr_schedule: the multiplier of the iteration in one device float that every Adam launch reads; None = nothing exists
        self.lr_schedule = lr_schedule.make_schedule(opt, device, self.optimizers())
        self.validation = validate.make(opt, device)   # --val_every, rank 0: the held-out stream and the history; else None
        self.frame_loss = frame_loss.make(opt)   # --frame_loss / --gdl_weight: the spec; None = the reference's MSE, nothing else exists
        self.frame_terms = self.frame_loss and frame_loss.FrameTerms(self.frame_loss, device)   # the terms + the epoch line's device sums

    def _step(self, optimizers):
        """A step site: the optimisers that step together after one backward pass (with several ranks: after the all-reduce
        of their ranges).  With a guard, ONE norm over all their gradients decides the clip factor or the skip."""
        guarded_step(optimizers, self.guard)

    # ---- data-parallel switches / statistics (bench.py's training leg) --------------------------
    def _ar(self, *actions):
        """Gradient all-reduce actions at this point of the iteration: ("reduce", (lo, hi)) | ("start", key, (lo, hi)) |
        ("finish", key) on ranges of the flat gradient arena.  Normally run at once; while a SegmentedIteration captures,
        the graph is cut here instead and the actions are replayed eagerly between the graph segments."""
        if self._segmenter is not None:
            if self.reducer.active():
                self._segmenter.cut(actions)
            return
        self._run_ar(actions)

    def _run_ar(self, actions):
        pend = self._ar_pending
        for a in actions:
            if a[0] == "reduce":
                self.reducer.reduce(*a[1])
            elif a[0] == "start":
                pend[a[1]] = self.reducer.start(*a[2])
            else:
                self.reducer.finish(pend.pop(a[1], None))

    def set_allreduce(self, on: bool):
        self.reducer.enabled = bool(on)

    def reset_allreduce_stats(self):
        self.reducer.calls = self.reducer.floats = 0
        self._iters = 0

    def allreduce_stats(self):
        """Collectives and bytes per iteration, and their standalone duration (parallel.allreduce_stats)."""
        return parallel.allreduce_stats(self, self._iters)

    # ---- mode switches (train.py:342-346,372-374) -------------------------------------------
    def train_mode(self):
        for m in self.modules:
            m.train()

    def _latent_stream(self):
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream()
            from dvg_amd import autograd as _ag
            _ag.JOIN_STREAMS.append(self._side_stream)   # the end-of-backward weight-gradient flush waits for it
        return self._side_stream

    def _lstm_seq_applies(self):
        from dvg_amd.models.lstm import sequence_applies
        return (self.lstm_sequence and self.time_batched and self.frame_predictor.training and torch.is_grad_enabled()
                and sequence_applies(self.frame_predictor))

    def _skip_rule(self, i, enc_out, skip):
        """train.py:158-161,184-187,217-220: skip is refreshed only while i < n_past (or last_frame_skip)."""
        if self.opt.last_frame_skip or i < self.opt.n_past:
            return enc_out[0], enc_out[1]
        return enc_out[0], skip

    # ---- the three closures -------------------------------------------------------------------
    def _encode_sequence(self, x, grad: bool):
        """encoder(x[t]) for every frame of the sequence, ONCE per frame.  The reference encodes every middle frame twice
        per closure (train.py:158-162,184-188,217-221: as step i's target and again as step i+1's input) with the same
        weights and the same batch, i.e. with identical outputs; one pass whose output is used twice gives the same
        losses and - autograd sums the two uses - the same gradients, and `fused.bn_passes(2)` reproduces the BatchNorm
        side effect of the second pass (two momentum updates, num_batches_tracked += 2) in the reference's order.
        (6S encoder passes per iteration become 3(S+1).)"""
        T = self.opt.n_past + self.opt.n_future
        if self.time_batched and self.encoder.training and T >= 3:
            return self._encode_sequence_batched(x, grad, T)
        outs = []
        with torch.set_grad_enabled(grad):
            for t in range(T):
                with fused.bn_passes(1 if (t == 0 or t == T - 1) else 2):
                    outs.append(self.encoder(x[t]))
        return outs

    def _encode_sequence_batched(self, x, grad: bool, T: int):
        """The T encoder calls of a closure as ONE pass over T x B frames.  train.py:213-221 is teacher-forced - every call
        encodes a ground-truth frame - so the calls are independent of each other; what ties a reference call together is
        its BatchNorm batch, and that is kept: statistics, normalisation and their backward are per GROUP of B consecutive
        images (one group per frame), and the running statistics advance frame by frame in the reference's order with the
        pass counts of the per-frame path (first / last frame once, middle frames twice).  Same losses, gradients and
        buffers up to fp32 summation order (tests/test_gpu_train.py); every conv launch is T x larger."""
        from dvg_amd.autograd import split_batch
        with torch.set_grad_enabled(grad), fused.bn_groups(T, (1, 2, 1)):
            h_all, skips_all = self.encoder(frames_as_batch(list(x[:T])))
        hs = split_batch(h_all, T)
        sks = [split_batch(s, T) for s in skips_all]
        return [(hs[t], [sk[t] for sk in sks]) for t in range(T)]

    def _share_scope(self):
        import contextlib
        return fused.share_skip_halves() if self.share_skip_halves else contextlib.nullcontext()

    def _enc(self, enc_all, x, t, grad=True):
        if enc_all is not None:
            return enc_all[t]
        with torch.set_grad_enabled(grad):
            return self.encoder(x[t])

    # Each closure has a `_dev` form that returns device tensors and never synchronises with the host, so that a whole
    # iteration can be captured into one hipGraph (train_graphs.GraphedIteration); the public forms add the float()s.
    def train_GP_Frame_predictor(self, x):
        return float(self._train_gp_dev(x)) / (self.opt.n_past + self.opt.n_future)

    def _loss_weights(self, dev, n_call, D):
        """[0.001 / n, 1000 / n, 0.001 / n, 0.01, -0.0001 x D]: train.py:239's weights on (sum sq mse, ae_mse, mse_gp, mse_latent,
        the D = S x g_dim entries of elbo) - max_ll = -elbo -; its tail [4:] is d loss / d elbo."""
        key = (dev, n_call, D)
        w = self._loss_w.get(key)
        if w is None:
            w = torch.tensor([0.001 / n_call, 1000.0 / n_call, 0.001 / n_call, 0.01] + [-0.0001] * D, dtype=torch.float32, device=dev)
            if not torch.cuda.is_current_stream_capturing():    # a tensor made during a capture lives in the graph's pool
                self._loss_w[key] = w                           # (ADVICE r05): never handed to later eager iterations
        return w

    def train_frame_predictor(self, x):
        return float(self._train_fp_dev(x)) / (self.opt.n_past + self.opt.n_future)

    def train_model(self, x):
        mse_latent, loss = self._train_model_dev(x)
        v = float(mse_latent) / (self.opt.n_past + self.opt.n_future)
        self.last_loss = float(loss)
        return v, v

    def _train_gp_dev(self, x, defer_step=False):
        opt = self.opt
        zero_grads([self.optimizer])
        self.frame_predictor.hidden = None      # train.py:150 re-creates it here, but this closure never steps the LSTM
        max_ll = 0
        skip = None
        g = self.finetune_encoder_grad
        cache, self._ft_cache = self._ft_cache, None
        if (cache is not None and cache[0] is x and not g and self.encoder.training and
                cache[3] == _derived.version_key(*self.encoder.parameters())):
            enc_all = cache[1]                       # same frames, same encoder weights: identical encodings ...
            fused.replay_bn_trace(cache[2])          # ... and the BatchNorm side effects of re-encoding them, replayed
        else:
            enc_all = self._encode_sequence(x, g) if self.share_encoder_passes else None
        if self.time_batched and enc_all is not None and not g and self.gp_layer.training:
            # no recurrence in this closure: all S GP posteriors + ELBO terms as one launch (gp_autograd.gp_elbo_steps)
            from dvg_amd.gp_autograd import gp_elbo_steps
            hcat = torch.stack([e[0].detach() for e in enc_all])          # (T, B, D)
            elbo, _ = gp_elbo_steps(self.gp_layer, self.mll, hcat[:-1], hcat[1:])
            if self.fused_losses:     # loss = (-elbo).sum(): d loss / d elbo = -1, no scalar graph
                gneg = self._loss_w.get(("neg1", elbo.device, elbo.numel()))
                if gneg is None:
                    gneg = torch.full((elbo.numel(),), -1.0, device=elbo.device)
                    if not torch.cuda.is_current_stream_capturing():   # as _derived.zero_state: a tensor first made during a
                        self._loss_w[("neg1", elbo.device, elbo.numel())] = gneg   # capture is written only when that graph replays
                loss = torch.dot(elbo.detach(), gneg)
                elbo.backward(gneg)
                if not defer_step:
                    self._ar(("reduce", self.rng_gp))
                    self._step([self.optimizer])
                return loss
            max_ll = -elbo
        else:
            for i in range(1, opt.n_past + opt.n_future):
                # Only the GP optimiser steps after this closure (train.py:170-171): the reference back-propagates into
                # the encoder and then discards those gradients (encoder.zero_grad() opens the next train_model).  The
                # encoder therefore runs without autograd here - same outputs, same BatchNorm running-stat updates, same
                # parameter updates, none of the wasted encoder backward.
                h, skip = self._skip_rule(i, self._enc(enc_all, x, i - 1, g), skip)
                h_target = self._enc(enc_all, x, i, g)[0].detach()
                h_pred = self.gp_layer(gp_input(self.gp_layer, h))
                max_ll = max_ll - self.mll(h_pred, h_target.transpose(0, 1))
        loss = max_ll.sum()
        loss.backward()
        if not defer_step:
            self._ar(("reduce", self.rng_gp))
            self._step([self.optimizer])
        return loss.detach()

    def _train_fp_dev(self, x, defer_step=False):
        opt = self.opt
        zero_grads([self.frame_predictor_optimizer])   # frame_predictor.zero_grad() (train.py:176): one fill of the flat range
        self.frame_predictor.hidden = None               # (re-created below by the step-by-step path; the sequence form starts
        #                                                   from its own zero state and leaves None behind)
        mse_latent = 0
        skip = None
        g = self.finetune_encoder_grad   # only frame_predictor_optimizer steps (train.py:195-196)
        self._ft_cache = None
        if self.share_encoder_passes and self.share_closure_encodings and not g:
            # the GP closure that follows encodes the same frames with the same encoder weights: keep the encodings and
            # the BatchNorm statistics of these passes for it (fused.bn_trace / replay_bn_trace)
            with fused.bn_trace() as trace:
                enc_all = self._encode_sequence(x, False)
            self._ft_cache = (x, enc_all, trace.entries, _derived.version_key(*self.encoder.parameters()))
        else:
            enc_all = self._encode_sequence(x, g) if self.share_encoder_passes else None
        if self._lstm_seq_applies() and enc_all is not None and not g:
            # teacher-forced: all S inputs exist before the recurrence starts - the sequence in one pass
            from dvg_amd.models.lstm import forward_sequence
            hcat = torch.stack([e[0].detach() for e in enc_all])              # (T, B, D)
            pred = forward_sequence(self.frame_predictor, hcat[:-1])
            if self.fused_losses:     # the sum of squares and its gradient in one launch; backward starts from d mse / d pred
                from dvg_amd import ops
                sq, d_pred = ops.mse_sum_grad(pred.detach(), hcat[1:], 1.0 / float(hcat[0].numel()))
                mse_latent = sq / float(hcat[0].numel())
                pred.backward(d_pred)
                if not defer_step:
                    self._ar(("reduce", self.rng_fp))
                    self._step([self.frame_predictor_optimizer])
                return mse_latent
            d = pred - hcat[1:]
            mse_latent = (d * d).sum() / float(hcat[0].numel())                # sum over the steps of nn.MSELoss (mean)
        else:
            self.frame_predictor.hidden = self.frame_predictor.init_hidden()       # train.py:178
            for i in range(1, opt.n_past + opt.n_future):
                h, skip = self._skip_rule(i, self._enc(enc_all, x, i - 1, g), skip)
                h_target = self._enc(enc_all, x, i, g)[0]
                h_pred = self.frame_predictor(h)
                mse_latent = mse_latent + self.mse_latent_criterion(h_pred, h_target)
        mse_latent.backward()
        if not defer_step:
            self._ar(("reduce", self.rng_fp))
            self._step([self.frame_predictor_optimizer])
        return mse_latent.detach()

    def _train_model_batched(self, x):
        """train_model (train.py:200-248) with the encoder AND decoder calls time-batched.  The closure is teacher-forced:
        step i reads the encodings of the ground-truth frames x[i-1], x[i]; so (1) all T frames are encoded in one pass
        (grouped BatchNorm, _encode_sequence_batched); (2) the latent chain - LSTM step, GP posterior + ELBO term, latent
        MSE, the only part with a recurrence - runs step by step on slices of those encodings; (3) the 3 S decoder calls
        (x_pred, x_target_pred, x_pred_gp for every step, :227-232) run as ONE decoder pass over 3 S B latents in the
        reference's call order, BatchNorm per call (group), with the skip tensors as SHARED BLOCKS: the three calls of a
        step read the same skip, and from step n_past on the skip is frozen (:217-220), so the skip half of every concat
        conv is computed (and back-propagated) once per DISTINCT skip - n_past - 1 times, not 3 S times.  Losses, gradients
        and buffers equal the step-by-step path up to fp32 summation order (tests/test_gpu_train.py)."""
        from dvg_amd import ops
        from dvg_amd.autograd import split_batch
        opt = self.opt
        T = opt.n_past + opt.n_future
        S = T - 1
        B = x[0].shape[0]
        # encoder / decoder / frame_predictor .zero_grad() (train.py:201-203) - adjacent ranges of the gradient arena: one fill
        zero_grads([self.encoder_optimizer, self.decoder_optimizer, self.frame_predictor_optimizer] +
                   ([] if self.reference_gp_grad_leak else [self.optimizer]))
        self.frame_predictor.hidden = None    # (the step-by-step branch below re-creates it; the sequence form never reads it)
        frames = frames_as_batch(list(x[:T]))
        with fused.bn_groups(T, (1, 2, 1)):
            h_all, skips_all = self.encoder(frames)
        staged = self.staged_backward
        if staged:     # cut the graph at the encoder outputs (see _train_model_dev)
            h_leaf = h_all.detach().requires_grad_(True)
            sk_leaf = [s.detach().requires_grad_(True) for s in skips_all]
        else:
            h_leaf, sk_leaf = h_all, list(skips_all)
        hs = split_batch(h_leaf, T)
        # the GP posterior + ELBO term of all S steps (no recurrence there: step i reads h(x[i-1]), h(x[i])): one launch
        from dvg_amd.gp_autograd import gp_elbo_steps
        D = h_leaf.shape[1]
        elbo, gp_means = gp_elbo_steps(self.gp_layer, self.mll, h_leaf[:S * B].view(S, B, D), h_leaf[B:].view(S, B, D))
        max_ll = -elbo
        # latent chain (the only recurrence): the LSTM steps
        fused_losses = self._lstm_seq_applies() and self.fused_losses
        if self._lstm_seq_applies():
            from dvg_amd.models.lstm import forward_sequence
            tgt_h = h_leaf[B:].view(S, B, D)
            pred = forward_sequence(self.frame_predictor, h_leaf[:S * B].view(S, B, D))      # (S, B, D)
            if fused_losses:     # sum of squares + its gradient in one launch (the scalar graph of :223,239 is not built)
                lat_sq, d_pred = ops.mse_sum_grad(pred.detach(), tgt_h.detach(), 0.01 / float(B * D))
                mse_latent = lat_sq / float(B * D)
            else:
                dlat = pred - tgt_h
                mse_latent = (dlat * dlat).sum() / float(B * D)                                  # sum over the steps of nn.MSELoss
            vec_all = torch.stack([pred, tgt_h, gp_means], 1).reshape(3 * S * B, D)              # reference call order
        else:
            self.frame_predictor.hidden = self.frame_predictor.init_hidden()       # train.py:206
            mse_latent = 0
            vecs = []
            for i in range(1, T):
                h, h_target = hs[i - 1], hs[i]
                h_pred = self.frame_predictor(h)
                mse_latent = mse_latent + self.mse_latent_criterion(h_pred, h_target)
                vecs += [h_pred, h_target, gp_means[i - 1]]
            vec_all = torch.cat(vecs, 0)                              # (3 S B, g_dim), reference call order
        # skip of step i: the encoder's skips of frame i-1 while i < n_past (or always with last_frame_skip), frozen after
        nblk = S if opt.last_frame_skip else max(1, opt.n_past - 1)
        gmap = tuple(min(g // 3, nblk - 1) for g in range(3 * S))
        mdev = ops.shared_map(gmap, vec_all.device)
        shared = [ops.SharedBlocks(s[:nblk * B], B, mdev, gmap) for s in sk_leaf]
        with fused.bn_groups(3 * S, (1, 1, 1)):
            x_all = self.decoder([vec_all, shared])               # (3 S B, nc, H, W)
        if fused_losses:
            # loss = 1000 ae_mse + 0.001 mse + 0.01 mse_latent + 0.001 mse_gp + 0.0001 max_ll.sum() (train.py:239) WITHOUT its
            # scalar autograd graph: the three frame terms' sums of squares and d loss / d x_all in one pass over the 3 S decoder
            # outputs (ops.frame_losses; call order x_pred, x_target_pred, x_pred_gp = mse, ae_mse, mse_gp), the latent term's
            # above, d loss / d elbo = -0.0001; backward starts from those seeds.  ~40 elementwise / reduction launches of torch
            # per iteration (two of them passes over all 3 S B frames) become 3.
            n_call = float(frames[0].numel() * B)
            if self.frame_loss is None:
                sq, d_x = ops.frame_losses(x_all.detach().view(S, 3, -1), frames[B:].view(S, -1),
                                           (0.001 / n_call, 1000.0 / n_call, 0.001 / n_call))
            else:     # --frame_loss / --gdl_weight: the same pass with another penalty and the edge terms (dvg_frame_losses_ext)
                sq, d_x = self.frame_terms.fused(x_all.detach(), frames[B:], S, B)
            wv = self._loss_weights(x_all.device, n_call, elbo.numel())       # elbo: one entry per (step, latent dim)
            loss = torch.dot(torch.cat([sq, mse_latent.view(1), elbo.detach()]), wv)
            torch.autograd.backward([x_all, pred, tgt_h, elbo], [d_x.view_as(x_all), d_pred, -d_pred, wv[4:]])
        else:
            tgt = frames[B:].view(S, 1, B, *frames.shape[1:])
            if self.frame_loss is None:
                per = x_all.view(S, 3, B, *frames.shape[1:]) - tgt
                # nn.MSELoss per call, summed over the steps = sum of squares / elements per call
                sq = (per * per).sum((0, 2, 3, 4, 5)) / float(per[0, 0].numel())
                mse, ae_mse, mse_gp = sq[0], sq[1], sq[2]
            else:     # --frame_loss / --gdl_weight as torch ops (frame_loss.torch_terms)
                mse, ae_mse, mse_gp = self.frame_terms.torch_calls(x_all.view(S, 3, B, *frames.shape[1:]), tgt[:, 0])
            loss = 1000 * ae_mse + 0.001 * mse + 0.01 * mse_latent + 0.001 * mse_gp + 0.0001 * max_ll.sum()
            loss.backward()
        self._encoder_backward_and_step(
            [(h_all, h_leaf.grad)] + [(s, l.grad) for s, l in zip(skips_all, sk_leaf) if l.grad is not None] if staged else None)
        return mse_latent.detach(), loss.detach()

    def _encoder_backward_and_step(self, pairs):
        """The end of train_model (train.py:240-245).  pairs: with the staged backward, (encoder output, gradient of the loss
        with respect to it) for every output the decoder / LSTM / GP phase reached; None: backward() went all the way."""
        if pairs is not None:
            # gradients of GP, likelihood, LSTM and decoder are final: their all-reduce runs under the encoder phase
            self._ar(("start", "a", (self.rng_gp[0], self.rng_dec[1])))
            torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
            self._ar(("start", "b", self.rng_enc), ("finish", "a"), ("finish", "b"))
        else:
            self._ar(("reduce", (self.rng_gp[0], self.rng_enc[1])))
        self._step([self.frame_predictor_optimizer, self.encoder_optimizer, self.decoder_optimizer, self.optimizer])

    def _train_model_dev(self, x):
        opt = self.opt
        if (self.time_batched and self.time_batched_decoder and self.share_encoder_passes and self.encoder.training
                and self.decoder.training and opt.n_past >= 2 and opt.n_past + opt.n_future >= 3):
            return self._train_model_batched(x)
        self.encoder_optimizer.zero_grad()            # encoder / decoder / frame_predictor .zero_grad() (train.py:201-203)
        self.decoder_optimizer.zero_grad()
        self.frame_predictor_optimizer.zero_grad()
        if not self.reference_gp_grad_leak:
            self.optimizer.zero_grad()                # the reference does NOT do this (see train.py's docstring)
        self.frame_predictor.hidden = self.frame_predictor.init_hidden()
        mse = mse_latent = mse_gp = ae_mse = 0
        max_ll = 0
        skip = None
        enc_all = self._encode_sequence(x, True) if self.share_encoder_passes else None
        staged = enc_all is not None and self.staged_backward
        if staged:
            # cut the graph at the encoder outputs: the decoder / LSTM / GP phase back-propagates into detached leaves,
            # whose gradients then seed the encoder phase (same sums, same gradients)
            enc_out = enc_all
            enc_all = [(h.detach().requires_grad_(True), [s.detach().requires_grad_(True) for s in sk])
                       for h, sk in enc_out]
        # The latent path (LSTM step, GP posterior + ELBO term, latent MSE: a few dozen small latency-bound kernels per
        # step) runs on a second stream, ahead of the decoder calls it feeds: the decoders' MFMA-bound kernels hide it.
        # autograd replays the stream assignment in the backward pass (a node runs on its forward stream, with event
        # dependencies); the end-of-backward weight-gradient flush and this function join the streams explicitly.
        cur = torch.cuda.current_stream()
        # (eager iterations only: replayed as a hipGraph the two-stream DAG measured 3-5 ms SLOWER per iteration - the
        # cross-stream dependency edges cost more than the overlap of kernels that no longer wait for the CPU gives; also at
        # the small per-GPU batches of the data-parallel shapes: 32.9 -> 35.3 ms (C4 dcgan_64), 50.4 -> 54.4 (C5 dcgan_128))
        side = self._latent_stream() if self.latent_stream and not torch.cuda.is_current_stream_capturing() else None
        for i in range(1, opt.n_past + opt.n_future):
            h, skip = self._skip_rule(i, self._enc(enc_all, x, i - 1), skip)
            h_target = self._enc(enc_all, x, i)[0]
            if side is not None:
                side.wait_stream(cur)          # this step's encodings (already there when the frames were encoded up front)
            with torch.cuda.stream(side if side is not None else cur):
                h_pred = self.frame_predictor(h)
                mse_latent = mse_latent + self.mse_latent_criterion(h_pred, h_target)
                gp_pred = self.gp_layer(gp_input(self.gp_layer, h))
                max_ll = max_ll - self.mll(gp_pred, h_target.transpose(0, 1))
                gp_mean = gp_pred.mean.transpose(0, 1)
            if side is not None:
                cur.wait_event(side.record_event())
                # ORDERING INVARIANT: everything the main stream consumes from the side stream was allocated BY the side
                # stream; the caching allocator only knows the allocating stream, so tell it about the consumer - a block
                # freed (in backward: by the main stream's nodes) must not be handed out again on the side stream while
                # main-stream kernels still read it.  (Until r03 safety rested on the wait_stream at the top of each step.)
                for t_ in (h_pred, gp_mean):
                    t_.record_stream(cur)
            with self._share_scope():   # the three decoder calls of a step share the skip halves of their concat convs
                x_pred = self.decoder([h_pred, skip])
                x_target_pred = self.decoder([h_target, skip])
                x_pred_gp = self.decoder([gp_mean, skip])
            if self.frame_loss is None:
                ae_mse = ae_mse + self.mse_latent_criterion(x_target_pred, x[i])
                mse = mse + self.mse_criterion(x_pred, x[i])
                mse_gp = mse_gp + self.mse_latent_criterion(x_pred_gp, x[i])
            else:     # --frame_loss / --gdl_weight as torch ops, one step
                mse, ae_mse, mse_gp = self.frame_terms.torch_step((mse, ae_mse, mse_gp), (x_pred, x_target_pred, x_pred_gp), x[i])
        if side is not None:
            cur.wait_stream(side)
        loss = 1000 * ae_mse + 0.001 * mse + 0.01 * mse_latent + 0.001 * mse_gp + 0.0001 * max_ll.sum()
        loss.backward()
        if side is not None:
            cur.wait_stream(side)              # the latent path's backward kernels
        self._encoder_backward_and_step(
            [(t, d.grad) for (h, sk), (hd, skd) in zip(enc_out, enc_all) for t, d in [(h, hd)] + list(zip(sk, skd))
             if d.grad is not None] if staged else None)
        return mse_latent.detach(), loss.detach()

    def _finetune_dev(self, x):
        """Both fine-tuning closures of an iteration (train.py:175-198 then :146-172).  They are independent of each other: the
        LSTM closure reads the encoder and the LSTM and steps only the LSTM, the GP closure reads the encoder and the GP and
        steps only the GP, and neither steps the encoder.  So both backward passes run first, then ONE all-reduce over the
        adjacent arena ranges [GP | likelihood | LSTM] (r06: was one collective - and one cut of the hipGraph chain - per
        closure), then both Adam steps: the same arithmetic as the reference's order, three collectives and four graph
        segments per data-parallel iteration instead of four and five."""
        fp = self._train_fp_dev(x, defer_step=True)
        gp = self._train_gp_dev(x, defer_step=True)
        self._ar(("reduce", (self.rng_gp[0], self.rng_fp[1])))
        self._step([self.frame_predictor_optimizer, self.optimizer])
        return fp, gp

    def finetune_temporal_encoders(self, x):
        fp, gp = self._finetune_dev(x)
        return (float(fp) + float(gp)) / (self.opt.n_past + self.opt.n_future)

    def optimizers(self):
        return [self.frame_predictor_optimizer, self.encoder_optimizer, self.decoder_optimizer, self.optimizer]

    def iteration(self, x):
        """One iteration of the training loop (train.py:354-361): train_model, then the two fine-tuning closures when
        opt.ft.  Returns (mse_ctrl, indices, temp_loss) as Python floats."""
        return self._iteration_result(self._iteration_dev(x))

    def _iteration_dev(self, x):
        """The device side of an iteration, the same launches eager or captured (GraphedIteration._body): nothing here reads
        a value back to the host.  Returns (mse_latent, loss, fp, gp) as device tensors; fp and gp are None without opt.ft."""
        self.lr_schedule is None or self.lr_schedule.tick()   # first: all step sites of the iteration read one multiplier
        mse_latent, loss = self._train_model_dev(x)
        fp, gp = self._finetune_dev(x) if self.opt.ft else (None, None)
        self.ema is None or self.ema.update()   # after the last step site of the iteration
        return mse_latent, loss, fp, gp

    def _iteration_result(self, outs):
        """The host side of an iteration, after its launches or the replay of their graph: the one place that reads the
        iteration's scalars back (train.py:361-362).  Sets last_loss and counts the iteration."""
        mse_latent, loss, fp, gp = outs
        T = self.opt.n_past + self.opt.n_future
        v = float(mse_latent) / T
        self.last_loss = float(loss)
        temp_loss = (float(fp) + float(gp)) / T if self.opt.ft else 0
        self._iters += 1
        return v, v, temp_loss

    # ---- qualitative rollout of train.py:256-289; write_plot below turns its result into the figures of :291-335 ------
    @torch.no_grad()
    def plot(self, x, epoch, nsample=5, eps_by_sample=None):
        """train.py:256-310 without the image writers: `nsample` rollouts whose ONE GP-sampled step is i == 10 (:281;
        the GP is fed the encoder output h, :283), then per batch row the sample with the smallest summed squared error
        (:303-310; ties keep the first sample, like the reference's strict `<`).  `eps_by_sample[s]`: base sample (D,B)
        of rollout s (parity runs); None = torch RNG.  Returns (gen (S,T,B,C,H,W), best (B,))."""
        opt = self.opt
        gen_seq = []
        for s in range(nsample):
            self.frame_predictor.hidden = self.frame_predictor.init_hidden()
            seq = [x[0]]
            x_in = x[0]
            skip = None
            for i in range(1, opt.n_eval):
                h, skip = self._skip_rule(i, self.encoder(x_in), skip)
                if i < opt.n_past:
                    if self.encoder.training:
                        # train.py:273-274 encodes x[i] and discards it; with the encoder left in train mode (:372-374) that
                        # call still updates the BatchNorm running statistics the checkpoint will carry
                        self.encoder(x[i])
                    self.frame_predictor(h)
                    x_in = x[i]
                else:
                    h_pred = self.frame_predictor(h)
                    if i == 10:  # train.py:281: the one GP-sampled step of the qualitative rollout
                        pred = self.likelihood(self.gp_layer(gp_input(self.gp_layer, h)))
                        z = pred.rsample(None if eps_by_sample is None else eps_by_sample[s])
                        x_in = self.decoder([z.transpose(0, 1), skip])
                    else:
                        x_in = self.decoder([h_pred, skip])
                seq.append(x_in)
            gen_seq.append(torch.stack(seq))
        gen = torch.stack(gen_seq)                       # (S,T,B,C,H,W)
        gt = torch.stack(list(x[:opt.n_eval]))           # (T,B,C,H,W)
        sse = ((gen - gt.unsqueeze(0)) ** 2).sum((1, 3, 4, 5))   # (S,B) — train.py:303-310 best-of-N
        return gen, sse.argmin(0)

    def write_plot(self, x, gen, best, epoch, out_dir):   # train.py:291-335: sample_<epoch>.png / .gif (viz.PlotWriter)
        self._plot_writer = self._plot_writer or viz.PlotWriter(getattr(self.opt, 'seed', 1))
        return self._plot_writer(x, gen, best, epoch, out_dir)

    def save(self, path):
        """train.py:380-388: whole-module pickles + GP / likelihood / GP-optimiser state dicts.  Every tensor written owns
        its storage: the live parameters, gradients and Adam moments are views of the shared FlatArena, and torch.save
        writes the whole storage behind a view (a checkpoint would carry the arena instead of the GP's moments, and loading
        only ck['encoder'] would pin all of it)."""
        torch.save(train_state.checkpoint(self), path)

    # ---- the whole training state (--resume): dvg_amd/train_state.py, docs/DESIGN_NOTES_resume.md --------------------
    def state_dict(self, epoch=0, train_gen=None, test_gen=None, shared=True):
        return train_state.capture(self, epoch, train_gen, test_gen, shared)

    def load_state_dict(self, sd, train_gen=None, test_gen=None, path="<state>"):
        return train_state.restore(self, sd, train_gen, test_gen, path)
