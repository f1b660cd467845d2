"""The inference rollout of generate_frames.py (the path the headline metric is quoted on).

`sample_rollout` is ONE pass of the `for s in range(nsample)` body of make_gifs
(generate_frames.py:143-177) with all five modules in eval mode:

    for i in 1..n_eval-1:
        h, skip = encoder(x_in)                 # skip kept only while i < n_past (or last_frame_skip)
        i <  n_past: step the LSTM on h, discard its output, x_in = x[i]          (:159-164)
        i >= n_past: h_pred = lstm(h)
                     i % 15 == 0: x_in = decoder([likelihood(gp(h^T)).rsample()^T, skip])   (:168-171)
                     else:        x_in = decoder([h_pred, skip])                            (:174)

The reference also runs `encoder(x[i])` on conditioning steps and discards it (:160-161); in eval
mode that call has no side effect, so it is skipped here.
Index bookkeeping (row K of SURVEY.md §8) is integer logic kept in `trigger_steps` / the skip rule.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _derived, fused, graphs, ops


# make_gifs: the prediction steps before the first GP trigger step once per batch instead of once per sample (GraphedSampler)
SHARE_PREFIX = True      # module attribute (tests toggle it; generate_frames.py --no_share_prefix); an environment switch until r06


def trigger_steps(n_past: int, n_eval: int, period: int = 15) -> List[int]:
    return [i for i in range(n_past, n_eval) if i % period == 0]


def frames_as_batch(frames):
    """The frames of a clip as ONE batch.  If they are consecutive contiguous slices of one buffer (data.batch_device(),
    GraphedRollout's static inputs) the batch is a view of it: no concat launch per rollout; a concat otherwise."""
    f0 = frames[0]
    step = f0.numel() * f0.element_size()
    st = f0.untyped_storage()
    for i, t in enumerate(frames):
        if (not t.is_contiguous() or t.shape != f0.shape or t.dtype != f0.dtype or
                t.untyped_storage().data_ptr() != st.data_ptr() or t.data_ptr() != f0.data_ptr() + i * step):
            return torch.cat(list(frames), 0)
    shape = (len(frames) * f0.shape[0],) + tuple(f0.shape[1:])
    return torch.as_strided(f0, shape, torch.empty(shape, device="meta").stride(), f0.storage_offset())


def gp_input(gp_layer, h):
    """The encoder / LSTM output h (B, D) as the GP layer's input (D, B, 1): one independent GP per latent dimension."""
    return h.transpose(0, 1).view(gp_layer.num_dims, h.shape[0], 1)


def _zero_hidden(frame_predictor):
    """init_hidden() (lstm.py:58-63) without its 2 x n_layers fill launches per rollout: one cached all-zero tensor per
    (device, batch, hidden size).  Safe to share: no kernel of the recurrent path writes its state in place (dvg_lstm_cell,
    dvg_gru_cell and dvg_rnn_cell reject in-place updates), and the tensors are only ever replaced in the `hidden` list.
    The predictor shapes the list (pairs for an LSTM, single tensors for a GRU / RNN: set_state_tensors)."""
    if not hasattr(frame_predictor, "step_state_only"):
        return frame_predictor.init_hidden()
    z = _derived.zero_state(frame_predictor.batch_size, frame_predictor.hidden_size, frame_predictor.embed.weight.device)
    if z is None:
        return frame_predictor.init_hidden()    # never cache a tensor that lives in a graph's private pool
    frame_predictor.set_state_tensors([z] * (frame_predictor.n_layers * frame_predictor.state_per_layer))
    return frame_predictor.hidden


# Skip tensors the rollout never reads are not stored (encoder.encode(x, skips_from), VggEncoder.features): of the conditioning
# batch only the LAST frame's skips survive, and once the skip is frozen (generate_frames.py:154-157) the encoder's skips of
# every predicted frame are discarded by the caller (`h, _ = h`).  ELIDE_SKIPS = False: every call stores all of them (module attribute; an environment switch until r06).
ELIDE_SKIPS = True


def _encode(encoder, x, skips_from=0):
    """encoder(x) -> (h, skips); with skips_from = k > 0 the skips hold the images [k, N) only (None when k == N)."""
    if skips_from and ELIDE_SKIPS and hasattr(encoder, "encode") and not encoder.training and not torch.is_grad_enabled():
        return encoder.encode(x, skips_from)
    h, skips = encoder(x)
    if skips_from:
        skips = [s[skips_from:] if skips_from < s.shape[0] else None for s in skips]
    return h, skips


def _encode_conditioning(encoder, x, n_past, last_frame_skip):
    """Eval-mode only: BatchNorm uses running statistics, so encoder outputs are independent across samples and the
    n_past-1 conditioning frames x[0..n_past-2] (all known before the rollout starts) can go through the encoder as
    ONE batch of B*(n_past-1) frames — bit-identical per-sample math, 9 passes' worth of launches folded into one and
    9x more tiles per launch for the deep 8x8 layers.  Returns ([h_1 .. h_{n_past-1}], skip of the last step)."""
    b = x[0].shape[0]
    last = n_past - 2     # the skips of the last frame x[n_past-2] alone (b images each)
    h_all, skip = _encode(encoder, frames_as_batch(x[:n_past - 1]), last * b)
    hs = [h_all[i * b:(i + 1) * b] for i in range(n_past - 1)]
    return hs, skip


def _step_discard(frame_predictor, h):
    """LSTM stepped on a conditioning frame, output discarded (generate_frames.py:125,162): skip the output GEMM."""
    if hasattr(frame_predictor, "step_state_only"):
        frame_predictor.step_state_only(h)
    else:
        frame_predictor(h)


@torch.no_grad()
def condition(encoder, frame_predictor, x: Sequence[torch.Tensor], n_past: int, last_frame_skip: bool = False,
              batch_conditioning: bool = True, decoder=None) -> dict:
    """The part of a sample rollout that does not depend on the sample (generate_frames.py:147-162 for i < n_past):
    the LSTM is reset and stepped on the encodings of the conditioning frames x[0..n_past-2] (outputs discarded), the
    skip tensors are those of x[n_past-2].  Deterministic in eval mode, so `make_gifs` (nsample rollouts of the SAME
    batch) computes it once per batch and draws every sample with `sample_from`."""
    frame_predictor.hidden = _zero_hidden(frame_predictor)
    skip = None
    hs = []
    if batch_conditioning and n_past >= 3 and not encoder.training:
        hs, skip = _encode_conditioning(encoder, x, n_past, last_frame_skip)
        side = None
        if (decoder is not None and not last_frame_skip and not decoder.training and fused.SKIP_HOIST and
                hasattr(decoder, "precompute_frozen_skips")):
            # The skip tensors are final here (generate_frames.py:154-157) and the LSTM warm-up below is a serial chain of
            # small latency-bound launches: the decoder's loop-invariant skip halves (fused._hoisted_skip) are computed
            # meanwhile on a second stream (a parallel branch of the hipGraph when captured) instead of on the critical
            # path of the first decoder call.
            side, cur = graphs.pooled_stream("hoist"), torch.cuda.current_stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                fused.declare_frozen_skips(skip)
                decoder.precompute_frozen_skips(skip)
        for i in range(1, n_past):
            _step_discard(frame_predictor, hs[i - 1])   # LSTM stepped on conditioning frames, output discarded (:162)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
    else:
        for i in range(1, n_past):
            h, skip = encoder(x[i - 1])
            hs.append(h)
            _step_discard(frame_predictor, h)
    # latents[i - 1] = enc(x[i - 1]), the latent fed at step i < n_past: what a VarianceTrigger records of the conditioning steps
    return {"hidden": list(frame_predictor.hidden), "skip": skip, "frames": [x[i] for i in range(n_past)], "latents": list(hs)}


def _predict_from(state: dict, encoder, decoder, frame_predictor, n_past: int, n_eval: int, last_frame_skip: bool,
                  latent) -> List[torch.Tensor]:
    """The prediction steps n_past ... n_eval - 1 from a `condition()` state; latent(i, h, h_pred) is what step i decodes."""
    frame_predictor.hidden = list(state["hidden"])   # lstm_cell returns new tensors: the saved state is never mutated
    frames = list(state["frames"])
    skip = state["skip"]
    x_in = frames[n_past - 1]
    for i in range(n_past, n_eval):
        keep = last_frame_skip or skip is None
        h, sk = _encode(encoder, x_in, 0 if keep else x_in.shape[0])   # frozen skip: this frame's skips are discarded (:157)
        if keep:
            skip = sk
        if i == n_past and not last_frame_skip and not decoder.training:
            fused.declare_frozen_skips(skip)    # frozen from here on: decoder blocks hoist their skip halves now
        h_pred = frame_predictor(h)
        x_in = decoder([latent(i, h, h_pred), skip])
        frames.append(x_in)
    return frames


class VarianceTrigger:
    """The sampler's second trigger rule (generate_frames.py --trigger variance; docs/DESIGN_NOTES_trigger_rows.md): a row of
    the batch draws a GP sample at the prediction step where ITS OWN predictive-variance norm exceeds mean + coef * std of ITS
    OWN window of the last `window` values (the reference's GPtrigger_gen rule, generate_frames.py:231,288-289, per sequence),
    at most once every min_gap + 1 steps.  It changes WHEN a row draws, not what a draw does; the bookkeeping of a step is one
    launch (ops.gp_trigger_rows).  The object holds the three numbers; the device state of one rollout comes from `new_state`."""

    def __init__(self, window: int = 12, coef: float = 2.01, min_gap: int = 0):
        if not 1 <= int(window) <= 64:
            raise ValueError(f"VarianceTrigger: window must be in 1..64, not {window}")
        if int(min_gap) < 0:
            raise ValueError(f"VarianceTrigger: min_gap must be >= 0, not {min_gap}")
        self.window, self.coef, self.min_gap = int(window), float(coef), int(min_gap)

    def key(self):
        return (self.window, self.coef, self.min_gap)

    def can_draw(self) -> bool:
        """False where the rule cannot draw whatever the values: the largest population z-score of one element among W is
        sqrt(W - 1), so coef >= sqrt(W - 1) never draws (W = 1: never)."""
        return self.window > 1 and self.coef < (self.window - 1) ** 0.5

    def first_decision(self, n_past: int) -> int:
        """The first step that decides: a prediction step whose value slid a full window."""
        return max(n_past, self.window + 1)

    def new_state(self, B: int, n_eval: int, device) -> dict:
        """win (B,W) zeros, last (B,) int32 'never', values (n_eval,B) zeros, thresholds (n_eval,B) +inf, flags (n_eval,B) int32
        zeros - views of ONE buffer (`blob`), so that a state is copied with one launch (`copy_state`)."""
        W = self.window
        sizes = (B * W, B, n_eval * B, n_eval * B, n_eval * B)
        blob = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
        win, last, values, thr, flags = torch.split(blob, sizes)
        st = {"blob": blob, "win": win.view(B, W), "last": last.view(torch.int32), "values": values.view(n_eval, B),
              "thresholds": thr.view(n_eval, B), "flags": flags.view(torch.int32).view(n_eval, B)}
        st["last"].fill_(ops.TRIGGER_NEVER)
        st["thresholds"].fill_(float("inf"))
        return st

    @staticmethod
    def copy_state(dst: dict, src: dict) -> None:
        dst["blob"].copy_(src["blob"])

    def _launch(self, st, i, var, decide, sample_db=None, h_pred=None):
        return ops.gp_trigger_rows(var, st["win"], st["last"], st["values"], st["thresholds"], st["flags"],
                                   pos=min(i - 1, self.window), step=i, slot=i, decide=decide, coef=self.coef,
                                   min_gap=self.min_gap, sample_db=sample_db, h_pred=h_pred)

    def record(self, st: dict, i: int, var: torch.Tensor) -> None:
        """Step i >= 1 that does not decide: its value fills position i - 1 of every row's window or slides it."""
        self._launch(st, i, var, False)

    def decide(self, st: dict, i: int, var: torch.Tensor, sample_db: torch.Tensor, h_pred: torch.Tensor) -> torch.Tensor:
        """Step i >= first_decision(n_past): the latent (B,D) the step decodes, row by row the GP sample or h_pred."""
        return self._launch(st, i, var, True, sample_db, h_pred)

    def record_conditioning(self, st: dict, latents, gp_layer, likelihood) -> None:
        """The values of the conditioning steps 1 .. n_past - 1 from `condition()`'s latents: the variance only, no sample."""
        for i, h in enumerate(latents, start=1):
            self.record(st, i, likelihood(gp_layer(gp_input(gp_layer, h))).variance)


def trigger_rows_host(values, n_past: int, window: int, coef: float, min_gap: int = 0, follow=None, guard: float = 0.0,
                      followed=None):
    """The variance rule on the host, in numpy float32 with the reference's own calls (generate_frames.py:231,288-289), row by
    row: values (n_eval, B) float32 with row 0 unused -> (flags (n_eval, B) int32, thresholds (n_eval, B) float32, +inf where no
    decision is taken).  The cross-check of ops.gp_trigger_rows and the decision of make_gifs(host_loop=True).
    follow (n_eval, B) with guard > 0: a decision whose margin |value - threshold| / |threshold| is below `guard` takes
    follow's flag instead of its own (parity runs against the device; `followed`, a list, gets its (step, row))."""
    host = HostTriggerRows(values.shape[1], window, coef, min_gap)
    flags = np.zeros(values.shape, dtype=np.int32)
    thresholds = np.full(values.shape, np.inf, dtype=np.float32)
    for i in range(1, values.shape[0]):
        flags[i], thresholds[i] = host.step(i, values[i], i >= n_past, None if follow is None else follow[i], guard, followed)
    return flags, thresholds


class HostTriggerRows:
    """`trigger_rows_host` one step at a time: every row's window and the step of its last draw, on the host."""

    def __init__(self, B: int, window: int, coef: float, min_gap: int = 0):
        self.window, self.coef, self.min_gap = window, coef, min_gap
        self.ctx = [np.zeros(0, dtype=np.float32) for _ in range(B)]
        self.last = [None] * B

    def step(self, i: int, value_row, prediction_step: bool, follow=None, guard: float = 0.0, followed=None):
        """(flags (B,) int32, thresholds (B,) float32) of step i; value_row (B,) float32."""
        B = len(self.ctx)
        flags, thresholds = np.zeros(B, dtype=np.int32), np.full(B, np.inf, dtype=np.float32)
        for b in range(B):
            value, context_array = value_row[b], self.ctx[b]
            full = len(context_array) == self.window
            context_array = np.concatenate([context_array[1:] if full else context_array, [value]])
            self.ctx[b] = context_array
            if not (full and prediction_step):
                continue
            threshold = np.mean(context_array) + self.coef * np.std(context_array)
            draw = bool(value > threshold) and (self.last[b] is None or i - self.last[b] > self.min_gap)
            if follow is not None and abs(float(value) - float(threshold)) < guard * abs(float(threshold)):
                draw = bool(follow[b])
                if followed is not None:
                    followed.append((i, b))
            if draw:
                self.last[b] = i
            flags[b], thresholds[b] = int(draw), threshold
        return flags, thresholds


@torch.no_grad()
def sample_from(state: dict, encoder, decoder, frame_predictor, gp_layer, likelihood, n_past: int, n_eval: int,
                last_frame_skip: bool = False, period: int = 15,
                eps_by_step: Optional[Dict[int, torch.Tensor]] = None, trigger: Optional[VarianceTrigger] = None,
                trigger_state: Optional[dict] = None) -> List[torch.Tensor]:
    """The prediction phase of one sample (generate_frames.py:163-176), starting from a `condition()` state.
    trigger: None = the period rule above; a VarianceTrigger = every row draws when its own variance says so (`period` is then
    unused and eps_by_step[i], if given, is needed at every deciding step).  trigger_state: the rollout's device state
    (VarianceTrigger.new_state; a fresh one if None), where the logs are left; the conditioning values are recorded into it
    from state["latents"] - a state without that entry (GraphedSampler's prefix) says they, and every step before n_past,
    already are."""
    if trigger is not None:
        ts = trigger_state
        if ts is None:
            ts = trigger.new_state(state["frames"][0].shape[0], n_eval, state["frames"][0].device)
        if state.get("latents") is not None:
            trigger.record_conditioning(ts, state["latents"], gp_layer, likelihood)

        def rows(i, h, h_pred):
            pred = likelihood(gp_layer(gp_input(gp_layer, h)))
            if i <= trigger.window:                      # still filling: the variance only
                trigger.record(ts, i, pred.variance)
                return h_pred
            z = pred.rsample(None if eps_by_step is None else eps_by_step[i])    # (D,B); the same launch leaves the variance
            return trigger.decide(ts, i, pred.variance, z, h_pred)
        return _predict_from(state, encoder, decoder, frame_predictor, n_past, n_eval, last_frame_skip, rows)

    def latent(i, h, h_pred):
        if not (period and i % period == 0):
            return h_pred
        pred = likelihood(gp_layer(gp_input(gp_layer, h)))
        return pred.rsample(None if eps_by_step is None else eps_by_step[i]).transpose(0, 1)
    return _predict_from(state, encoder, decoder, frame_predictor, n_past, n_eval, last_frame_skip, latent)


@torch.no_grad()
def sample_rollout(encoder, decoder, frame_predictor, gp_layer, likelihood, x: Sequence[torch.Tensor], n_past: int,
                   n_eval: int, last_frame_skip: bool = False, period: int = 15,
                   eps_by_step: Optional[Dict[int, torch.Tensor]] = None,
                   batch_conditioning: bool = True) -> List[torch.Tensor]:
    """Returns the n_eval frames [x0, ..] of one sample (conditioning frames are the inputs themselves): one complete
    rollout = condition() + sample_from()."""
    state = condition(encoder, frame_predictor, x, n_past, last_frame_skip, batch_conditioning, decoder)
    return sample_from(state, encoder, decoder, frame_predictor, gp_layer, likelihood, n_past, n_eval, last_frame_skip,
                       period, eps_by_step)


@torch.no_grad()
def posterior_rollout(encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval,
                      last_frame_skip=False) -> List[torch.Tensor]:
    """generate_frames.py:110-134: the GP is fed the LSTM output and its predictive MEAN is decoded."""
    frame_predictor.hidden = frame_predictor.init_hidden()
    frames = [x[0]]
    x_in = x[0]
    skip = None
    for i in range(1, n_eval):
        keep = last_frame_skip or i < n_past
        h, sk = _encode(encoder, x_in, 0 if keep else x_in.shape[0])
        if keep:
            skip = sk
        if i == n_past and not last_frame_skip and not decoder.training:
            fused.declare_frozen_skips(skip)
        if i < n_past:
            _step_discard(frame_predictor, h)
            x_in = x[i]
        else:
            h_pred = frame_predictor(h)
            pred = likelihood(gp_layer(gp_input(gp_layer, h_pred)))
            x_in = decoder([pred.mean.transpose(0, 1), skip])
        frames.append(x_in)
    return frames


@torch.no_grad()
def posterior_from(state: dict, encoder, decoder, frame_predictor, gp_layer, likelihood, n_past: int, n_eval: int,
                   last_frame_skip: bool = False) -> List[torch.Tensor]:
    """`posterior_rollout`'s prediction steps n_past ... n_eval - 1 from a `condition()` state.  Its conditioning phase
    (generate_frames.py:113-121 for i < n_past: the encoder on x[i-1], the LSTM stepped with the output discarded, the skip
    tensors of the last such frame, x[i] handed on) is the same computation as the samples' (:147-162), so `make_gifs` runs it
    once for both."""
    return _predict_from(state, encoder, decoder, frame_predictor, n_past, n_eval, last_frame_skip,
                         lambda i, h, h_pred: likelihood(gp_layer(gp_input(gp_layer, h_pred))).mean.transpose(0, 1))


# ---- GPtrigger_gen (generate_frames.py:220-298) without a host round trip per step --------------------------------------------
# The reference pulls the predictive variance to the host at every step, slides the 12-long window in numpy and branches in
# Python; it re-runs the 12 warm-up steps for every batch index although only the COLUMN of the variance norms they record
# depends on the index (:275), and it encodes x_in two or three times per step (`var_value`, then `generation` or the trigger
# branch: the same eval-mode encoder on the same frame).  Here: the warm-up once per batch with the norms of every sample
# (`trigger_warmup`), one encoder call per step, the decision and the branch select on the device (ops.gp_trigger_step /
# gp_trigger_select: both branches' cheap parts - the GP sample, the LSTM step - are computed, the flag picks the latent to
# decode and the recurrent state that survives), so that the main loop is capturable (`GraphedTrigger`) and the value /
# threshold / trigger logs are read back once per index.
@torch.no_grad()
def trigger_warmup(encoder, decoder, frame_predictor, gp_layer, likelihood, x0, warmup: int = 12, skip_steps: int = 5) -> dict:
    """Loop steps 0 .. warmup-1 of GPtrigger_gen (:266-280) for the whole batch: autoregressive from x0, skip tensors of the steps
    i < skip_steps (:268-269), every step `generation` (:220-224).  norms[i, b] = the value the reference records at step i
    for batch index b (:275)."""
    b = x0.shape[0]
    frame_predictor.hidden = _zero_hidden(frame_predictor)
    x_in, skip, norms, frames = x0, None, [], []
    for i in range(warmup):
        keep = i < skip_steps
        h, sk = _encode(encoder, x_in, 0 if keep else b)
        if keep:
            skip = sk
        if i == skip_steps - 1 and not decoder.training:
            fused.declare_frozen_skips(skip)            # final from here on (:268-271)
        pred = likelihood(gp_layer(gp_input(gp_layer, h)))
        norms.append(ops.gp_var_norms(pred.variance))
        x_in = decoder([frame_predictor(h), skip])      # generation(): its encoder call is the one above (eval mode)
        frames.append(x_in)
    return {"x_in": x_in, "skip": skip, "hidden": list(frame_predictor.hidden), "norms": torch.stack(norms), "frames": frames}


@torch.no_grad()
def trigger_body(state: dict, encoder, decoder, frame_predictor, gp_layer, likelihood, ctx, coef: float, eps_all, log: dict,
                 warmup: int = 12, total: int = 105, probe: int = 3) -> List[torch.Tensor]:
    """Loop steps warmup .. total-1 (:285-297) from a `trigger_warmup` state.  ctx: the window (float32, device), initialised
    by the caller to norms[:, index] and slid in place; eps_all[i - warmup]: the base sample (D,B) of step i; log: device
    tensors `flag` (1 int32), `values` / `thresholds` (total float32), `flags` (total int32).  Nothing here syncs."""
    b = state["x_in"].shape[0]
    if b <= probe:
        raise IndexError(f"GPtrigger_gen reads sample [{probe}] of the batch (generate_frames.py:230): batch_size must be > {probe}")
    frame_predictor.hidden = list(state["hidden"])
    x_in, skip, frames = state["x_in"], state["skip"], []
    for i in range(warmup, total):
        h, _ = _encode(encoder, x_in, b)
        pred = likelihood(gp_layer(gp_input(gp_layer, h)))
        z = pred.rsample(eps_all[i - warmup])                       # (D,B); the same launch leaves the variance
        ops.gp_trigger_step(pred.variance, probe, ctx, coef, log["flag"], log["values"], log["thresholds"], log["flags"], i)
        old = frame_predictor.state_tensors()
        h_pred = frame_predictor(h)
        new = frame_predictor.state_tensors()
        vec, st = ops.gp_trigger_select(log["flag"], z, h_pred, old, new)
        frame_predictor.set_state_tensors(st)
        x_in = decoder([vec, skip])
        frames.append(x_in)
    return frames


def trigger_log(total: int, device) -> dict:
    return {"flag": torch.zeros(1, dtype=torch.int32, device=device), "values": torch.zeros(total, device=device),
            "thresholds": torch.zeros(total, device=device), "flags": torch.zeros(total, dtype=torch.int32, device=device)}


class GraphedTrigger:
    """GPtrigger_gen for one batch as two hipGraphs: the warm-up (once per batch) and the main loop (once per batch index; it
    reads the warm-up graph's state - frames, the predictor's recurrent state, skip tensors and the decoder's hoisted skip halves -
    and its own static window / base samples / logs).  `warm(x0)` then `run(index)`; one device-to-host copy of the logs per index."""

    def __init__(self, encoder, decoder, frame_predictor, gp_layer, likelihood, x0, warmup=12, total=105, depth=1,
                 skip_steps=5, probe=3):
        self._mods = (encoder, decoder, frame_predictor, gp_layer, likelihood)
        self.warmup, self.total, self.probe, self.skip_steps = warmup, total, probe, skip_steps
        self.coef = 2 + 0.01 * depth
        dev, b, d = x0.device, x0.shape[0], gp_layer.num_dims
        self.x0 = x0.contiguous().clone()
        self.eps = torch.zeros(max(1, total - warmup), d, b, device=dev)
        self.ctx = torch.zeros(warmup, device=dev)
        self.log = trigger_log(total, dev)
        graphs.warm_up(lambda: self._body(self._warm()[0]))
        with graphs.skip_scope():
            self.warm_graph, (self.state, self.warm_stack), self._keep_w = graphs.capture(self._warm)
            # (the skip-dependent cache entries the warm-up graph created stay while the body is captured: it reads those buffers)
            self.body_graph, self.body_stack, self._keep_b = graphs.capture(lambda: self._body(self.state))

    def _warm(self):
        st = trigger_warmup(*self._mods, self.x0, self.warmup, self.skip_steps)
        return st, torch.stack(st["frames"])

    def _body(self, st):
        fr = trigger_body(st, *self._mods, self.ctx, self.coef, self.eps, self.log, self.warmup, self.total, self.probe)
        return torch.stack(fr) if fr else None

    def warm(self, x0) -> None:
        self.x0.copy_(x0)
        self.warm_graph.replay()

    def run(self, index: int, eps_by_step: Optional[Dict[int, torch.Tensor]] = None) -> dict:
        """One batch index: frames (total,B,C,H,W) (static buffers: clone to keep), and on the host the trigger steps, the
        recorded values (total) and the thresholds (total - warmup)."""
        self.ctx.copy_(self.state["norms"][:, index])
        if eps_by_step is None:
            self.eps.normal_()
        else:
            for i in range(self.warmup, self.total):
                self.eps[i - self.warmup].copy_(eps_by_step[i])
        if self.body_stack is not None:
            self.body_graph.replay()
        values = torch.cat([self.state["norms"][:, index], self.log["values"][self.warmup:]]).cpu()
        thresholds = self.log["thresholds"][self.warmup:].cpu()
        flags = self.log["flags"][self.warmup:].cpu()
        frames = self.warm_stack if self.body_stack is None else torch.cat([self.warm_stack, self.body_stack])
        return {"frames": frames, "triggers": [self.warmup + int(i) for i in torch.nonzero(flags).flatten()],
                "values": [float(v) for v in values], "thresholds": [float(v) for v in thresholds],
                "values_main": self.log["values"][self.warmup:].clone()}


class GraphedRollout:
    """`sample_rollout` captured once into a hipGraph (torch.cuda.CUDAGraph) and replayed: the ~500 launches of
    a rollout (19 encoder + 10 decoder passes, 38 LSTM cells, GEMMs, the GP sample) are launch-latency-bound at
    small batch / for dcgan_64, and the per-step Python + ctypes cost disappears from the critical path.
    Inputs are copied into static buffers; the returned frames are static tensors overwritten by every replay
    (clone them to keep a sample).  The GP base samples eps (D,B) live in static buffers that every call refills from
    torch's generator on the replay stream, OUTSIDE the graph: a generator captured inside hands all graphs of a process
    the same device-side offset tensor, and two graphs replayed on different streams (ConcurrentRollouts) then read the
    same offset and draw the same sample."""

    def __init__(self, encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval,
                 last_frame_skip=False, period=15, warmup=2):
        self._args = (encoder, decoder, frame_predictor, gp_layer, likelihood)
        self._kw = dict(n_past=n_past, n_eval=n_eval, last_frame_skip=last_frame_skip, period=period)
        buf = torch.stack([t.contiguous() for t in x])      # one buffer: the conditioning batch is a view of it
        self.static_x = [buf[i] for i in range(len(x))]
        self.eps = {i: torch.randn(gp_layer.num_dims, x[0].shape[0], device=x[0].device)
                    for i in (trigger_steps(n_past, n_eval, period) if period else [])}
        self._kw["eps_by_step"] = self.eps
        run = lambda: sample_rollout(*self._args, self.static_x, **self._kw)   # noqa: E731
        graphs.warm_up(run, warmup)
        with graphs.skip_scope():
            self.graph, self.frames, self._keepalive = graphs.capture(run)

    def __call__(self, x: Optional[Sequence[torch.Tensor]] = None,
                 eps_by_step: Optional[Dict[int, torch.Tensor]] = None) -> List[torch.Tensor]:
        """`eps_by_step`: base samples (D,B) per trigger step (parity runs); None = fresh draws from torch's generator."""
        if x is not None:
            for dst, src in zip(self.static_x, x):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        for i, e in self.eps.items():
            if eps_by_step is None:
                e.normal_()
            else:
                e.copy_(eps_by_step[i])
        self.graph.replay()
        return self.frames


class ConcurrentRollouts:
    """`inflight` complete rollouts of ONE batch in flight at once: the rollouts of make_gifs' `for s in range(nsample)`
    loop (generate_frames.py:143-177) are independent of each other, so each gets its own hipGraph (own static buffers, own
    private pool: no buffer is shared between two graphs; weights, packed weights and BatchNorm folds are read-only) and its
    own stream.  A rollout is a serial chain of ~500 launches, many of them small (LSTM cells, GEMV-shaped ends, the GP
    sample, the 8x8 / 4x4 layers): with several chains in flight the tail of one launch and the latency-bound phases of one
    rollout fill with another rollout's work.  Per-rollout arithmetic is unchanged (every rollout is a full
    `sample_rollout`: conditioning included, nothing shared or amortised across rollouts) and so are its results.
    `run(n)` issues n rollouts round-robin over the graphs and returns the static frame lists of the `inflight` most
    recent ones; the caller synchronises (or records events) before reading them."""

    def __init__(self, encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval, inflight=2,
                 last_frame_skip=False, period=15, energy_tiles=None):
        if inflight < 1:
            raise ValueError("inflight must be >= 1")
        # Several chains in flight keep the board at its power cap: their graphs are captured under the ENERGY
        # tile policy (128 x 128 batched-GEMM tile, 8 x 16 pixel tiles from one workgroup per CU on: fewer LDS / L2 bytes per
        # MFMA, +4.6 % vgg_64); one chain keeps the latency tiles (`energy_tiles` overrides: profiling one chain of the in-flight
        # kernels).  The two policies' results agree to fp32 rounding, not bit for bit.
        self.energy_tiles = inflight >= 2 if energy_tiles is None else bool(energy_tiles)
        with ops.tile_policy(self.energy_tiles):
            self.rollouts = [GraphedRollout(encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval,
                                            last_frame_skip, period) for _ in range(inflight)]
        self.streams = [graphs.pooled_stream("chain", k) for k in range(inflight)]
        self._next = 0

    def run(self, n: int, x: Optional[Sequence[torch.Tensor]] = None, chains: Optional[int] = None) -> List[List[torch.Tensor]]:
        """`chains`: use only the first `chains` graphs (1 = the rollouts back to back as one serial chain)."""
        nc = len(self.rollouts) if chains is None else max(1, min(chains, len(self.rollouts)))
        cur = torch.cuda.current_stream()
        for s in self.streams[:nc]:
            s.wait_stream(cur)            # inputs written on the caller's stream are visible to every chain
        for _ in range(n):
            k = self._next % nc
            self._next = (k + 1) % nc
            with torch.cuda.stream(self.streams[k]):
                self.rollouts[k](x)       # a stream runs its replays in order: a graph never overlaps itself
        for s in self.streams[:nc]:
            cur.wait_stream(s)
        return [r.frames for r in self.rollouts[:nc]]


_TRIGGER_LOGS = ("flags", "values", "thresholds")


class GraphedSampler:
    """`make_gifs` for one batch (generate_frames.py:107-178) as hipGraphs.  Everything that does not depend on the sample is
    replayed once per batch (three graphs: the conditioning, then side by side the other two): the conditioning (`condition`: the past frames encoded as one batch, the LSTM warmed up,
    the decoder's loop-invariant skip halves), the posterior rollout's prediction steps (`posterior_from`, :110-134 - its
    conditioning phase is the same computation as the samples') and, with `share_prefix`, the samples' prediction steps before
    the first GP trigger step with their SSIM / PSNR.  The body of the `for s in range(nsample)` loop (:163-178) - the remaining
    steps of one sample and utils.eval_seq's metrics - is one graph per chain, replayed once per sample, `inflight` samples at
    a time (one graph + one stream each, see ConcurrentRollouts); the sample graphs read the batch graph's state and
    skip-dependent tensors (read-only during their replays); GP base samples eps (D,B) per trigger step, predicted frames
    and metrics are per chain.  `set_batch()` installs a new batch, `run()` replays.

    `share_prefix` (default: rollout.SHARE_PREFIX): the samples of a batch differ only from the first GP trigger step t0 on
    (generate_frames.py:166-171: the draw at i % 15 == 0 is the loop's only source of randomness), so the prediction steps
    n_past ... t0 - 1 - the same kernels on the same inputs for every sample, like the conditioning frames - run ONCE per
    batch and every sample graph continues from the state they leave behind.  Results are bit-identical to the per-sample
    loop (tests/test_gpu_rollouts.py); with no trigger step inside the rollout all samples are the prefix.

    `metrics`: "skimage" (default) scores with utils.eval_seq's metrics, one ops.eval_frames per step; "finn" with
    utils.finn_eval_seq's (ops.eval_frames_finn, one launch per captured step range), which adds the frames' MSE - `run()`
    then fills its `mse` output as well.  The frames do not depend on it."""

    def __init__(self, encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval,
                 last_frame_skip=False, period=15, inflight=3, share_prefix=None, metrics="skimage", trigger=None):
        if metrics not in ("skimage", "finn"):
            raise ValueError(f"GraphedSampler: metrics must be 'skimage' or 'finn', not {metrics!r}")
        self.metrics = metrics
        self.trigger = trigger
        # several sample chains in flight keep the board at its power cap: their graphs are captured with the energy-lean tiles
        # (ops.tile_policy; same results to fp32 rounding); one chain at a time keeps the latency tiles
        with ops.tile_policy(max(1, inflight) >= 2):
            self._init(encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval, last_frame_skip, period,
                       inflight, share_prefix)

    def _init(self, encoder, decoder, frame_predictor, gp_layer, likelihood, x, n_past, n_eval, last_frame_skip, period,
              inflight, share_prefix):
        self._mods = (encoder, decoder, frame_predictor, gp_layer, likelihood)
        self.n_past, self.n_eval, self.period = n_past, n_eval, period
        self.last_frame_skip = last_frame_skip
        self._kw = dict(last_frame_skip=last_frame_skip, period=period)
        dev = x[0].device
        B, D = x[0].shape[0], gp_layer.num_dims
        self.x = torch.stack([t.contiguous() for t in x])            # conditioning frames + ground truth of the metrics
        self.steps = [i for i in range(n_past, n_eval) if period and i % period == 0]
        trig = self.trigger
        if trig is not None:
            # every row decides for itself at every step from the first one whose value slid a full window: no row can draw
            # before it, so the steps up to there are still the same for every sample
            self.steps = list(range(trig.first_decision(n_past), n_eval))
            self._trig_init = trig.new_state(B, n_eval, dev)      # never written after this line: what a rollout starts from
            self._trig_pre = trig.new_state(B, n_eval, dev)       # the shared prefix's: conditioning values, then its steps'
        if share_prefix is None:
            share_prefix = SHARE_PREFIX
        self.t0 = min(self.steps) if self.steps else n_eval          # first step whose outcome depends on the sample
        self.share = bool(share_prefix) and self.t0 > n_past and not last_frame_skip and n_past >= 2
        if not self.share:
            self.t0 = n_past
        self.b = None
        self.chains = []
        for k in range(max(1, inflight)):
            self.chains.append({"eps": {i: torch.zeros(D, B, device=dev) for i in self.steps},
                                "stream": graphs.pooled_stream("chain", k),
                                "trig": None if trig is None else trig.new_state(B, n_eval, dev)})
        self.post_stream = graphs.pooled_stream("post")

        def eager():
            self.b = {"state": self._condition()}
            self.b["post"] = self._posterior()
            self.b["pre"] = self._prefix() if self.share else None
            self._body(self.chains[0])
        graphs.warm_up(eager)
        # Three graphs for the sample-independent part: the conditioning, then - independent of each other, replayed on two
        # streams - the posterior rollout's prediction steps and the samples' shared prefix.  The conditioning graph comes
        # first: the skip-dependent tensors it creates (hoisted skip halves) and those of the first decoder call after it (the
        # skip's share of the last projection) stay in the caches while the later graphs are captured, so those read buffers
        # written once per batch, before they replay, instead of recomputing them per sample.
        # What a graph added belongs to THAT graph's pool and replays: where the next capture must not see it, it is dropped.
        self.b = {}
        with graphs.skip_scope() as skips:
            self.cond_graph, self.b["state"], self._keep_c = graphs.capture(self._condition)
            after_cond = skips.mark()
            # the posterior graph replays BESIDE the prefix graph (another stream): it may read what the conditioning graph
            # wrote, never what the prefix graph writes
            self.post_graph, self.b["post"], self._keep_o = graphs.capture(self._posterior)
            skips.drop_since(after_cond)
            self.pre_graph, self.b["pre"] = None, None
            if self.share:
                self.pre_graph, self.b["pre"], self._keep_p = graphs.capture(self._prefix)
            main_stream = skips.mark()    # written by graphs that replay on the main stream before any sample graph
            for ch in (() if self.t0 == n_eval else self.chains):
                ch["graph"], (ch["frames"], ch["ssim"], ch["psnr"], ch["mse"]), ch["keepalive"] = \
                    graphs.capture(lambda: self._body(ch))
                skips.drop_since(main_stream)

    def _metrics(self, frames, lo, hi):
        """(ssim, psnr, mse), each (B, hi - lo), of the predicted frames lo ... hi - 1; mse is None unless metrics == "finn"
        (utils.finn_eval_seq: one launch for the whole step range)."""
        if self.metrics == "finn":
            s, p, e = ops.eval_frames_finn(self.x[lo:hi], torch.stack(frames[lo:hi]))
            return s.t(), p.t(), e.t()
        m = [ops.eval_frames(self.x[t], frames[t]) for t in range(lo, hi)]
        return torch.stack([a for a, _ in m], 1), torch.stack([b for _, b in m], 1), None

    def _condition(self) -> dict:
        """The conditioning state (rollout.condition) of the frames in self.x."""
        enc, dec, fp, gp, lik = self._mods
        return condition(enc, fp, [self.x[i] for i in range(self.x.shape[0])], self.n_past, self.last_frame_skip, decoder=dec)

    def _posterior(self) -> torch.Tensor:
        return torch.stack(posterior_from(self.b["state"], *self._mods, self.n_past, self.n_eval, self.last_frame_skip))

    def _prefix(self) -> dict:
        """The samples' steps n_past ... t0 - 1 from the conditioning state: frames, their metrics, the LSTM state after them."""
        st = self.b["state"]
        if self.trigger is not None:         # the conditioning steps' values and the prefix's own: every sample starts from them
            self.trigger.copy_state(self._trig_pre, self._trig_init)
            frames = sample_from(st, *self._mods, n_past=self.n_past, n_eval=self.t0, trigger=self.trigger,
                                 trigger_state=self._trig_pre, **self._kw)
        else:
            frames = sample_from(st, *self._mods, n_past=self.n_past, n_eval=self.t0, **self._kw)
        ssim, psnr, mse = self._metrics(frames, self.n_past, self.t0)
        return {"hidden": list(self._mods[2].hidden), "skip": st["skip"], "frames": frames, "stack": torch.stack(frames),
                "ssim": ssim, "psnr": psnr, "mse": mse}

    def _body(self, ch):
        """One sample from step t0 on: (frames t0 ... n_eval - 1 stacked - with the conditioning frames in front when there is
        no shared prefix -, SSIM, PSNR and - Finn metrics only, else None - MSE of the predicted ones among them)."""
        if self.t0 == self.n_eval:       # no trigger step inside the rollout: every sample IS the prefix
            return None, None, None, None
        state = self.b["pre"] if self.share else self.b["state"]
        if self.trigger is not None:
            # the chain's own window / last / logs, first set to what the rollout has recorded up to t0: the prefix's state (it
            # carries no "latents": nothing is recorded twice) or, without a shared prefix, the initial one
            self.trigger.copy_state(ch["trig"], self._trig_pre if self.share else self._trig_init)
            frames = sample_from(state, *self._mods, eps_by_step=ch["eps"], n_past=self.t0, n_eval=self.n_eval,
                                 trigger=self.trigger, trigger_state=ch["trig"], **self._kw)
        else:
            frames = sample_from(state, *self._mods, eps_by_step=ch["eps"], n_past=self.t0, n_eval=self.n_eval, **self._kw)
        ssim, psnr, mse = self._metrics(frames, self.t0, self.n_eval)
        return torch.stack(frames[self.t0 if self.share else 0:]), ssim, psnr, mse

    def set_batch(self, x) -> None:
        """New frames (conditioning + ground truth), copied into the static buffer on the current stream."""
        for i, t in enumerate(x):
            self.x[i].copy_(t)

    def run(self, nsample: int, samples: torch.Tensor, ssim: torch.Tensor, psnr: torch.Tensor,
            eps_by_sample: Optional[Sequence[Dict[int, torch.Tensor]]] = None,
            mse: Optional[torch.Tensor] = None, trigger_log: Optional[dict] = None) -> torch.Tensor:
        """Draws `nsample` samples: samples[s] <- the n_eval frames (n_eval,B,C,H,W), ssim[:, s] / psnr[:, s] <- (B,T); returns
        the posterior rollout's frames (n_eval,B,C,H,W) - a static buffer the next run() overwrites.
        eps_by_sample[s][i]: base sample of sample s at trigger step i (parity runs); None = torch's generator.
        mse (metrics == "finn" only): mse[:, s] <- (B,T), the frames' mean squared error.
        trigger_log (a sampler with a VarianceTrigger only): its 'flags' (int32), 'values' and 'thresholds', each (nsample, n_eval, B),
        get every sample's logs."""
        if trigger_log is not None and self.trigger is None:
            raise ValueError("GraphedSampler.run: a trigger log needs a sampler built with a VarianceTrigger")
        if (mse is not None) != (self.metrics == "finn"):
            raise ValueError("GraphedSampler.run: the mse output goes with metrics='finn', and only with it")
        cur = torch.cuda.current_stream()
        P = self.t0 - self.n_past
        self.cond_graph.replay()             # on the current stream: everything below waits for it
        self.post_stream.wait_stream(cur)
        with torch.cuda.stream(self.post_stream):
            self.post_graph.replay()         # beside the prefix and the samples (it only reads the conditioning state)
        if self.share:
            self.pre_graph.replay()
            pre = self.b["pre"]
            samples[:, :self.t0].copy_(pre["stack"].unsqueeze(0).expand(nsample, *pre["stack"].shape))
            ssim[:, :, :P].copy_(pre["ssim"].unsqueeze(1).expand(-1, nsample, -1))
            psnr[:, :, :P].copy_(pre["psnr"].unsqueeze(1).expand(-1, nsample, -1))
            if mse is not None:
                mse[:, :, :P].copy_(pre["mse"].unsqueeze(1).expand(-1, nsample, -1))
            if self.t0 == self.n_eval:
                if trigger_log is not None:
                    for k in _TRIGGER_LOGS:
                        trigger_log[k].copy_(self._trig_pre[k].unsqueeze(0).expand(nsample, -1, -1))
                cur.wait_stream(self.post_stream)
                return self.b["post"]
        for ch in self.chains:
            ch["stream"].wait_stream(cur)
        lo = self.t0 if self.share else 0
        for s in range(nsample):
            ch = self.chains[s % len(self.chains)]
            with torch.cuda.stream(ch["stream"]):
                for i in self.steps:
                    if eps_by_sample is None:
                        ch["eps"][i].normal_()
                    else:
                        ch["eps"][i].copy_(eps_by_sample[s][i])
                ch["graph"].replay()
                samples[s, lo:].copy_(ch["frames"])
                ssim[:, s, P:].copy_(ch["ssim"])
                psnr[:, s, P:].copy_(ch["psnr"])
                if mse is not None:
                    mse[:, s, P:].copy_(ch["mse"])
                if trigger_log is not None:
                    for k in _TRIGGER_LOGS:
                        trigger_log[k][s].copy_(ch["trig"][k])
        for ch in self.chains:
            cur.wait_stream(ch["stream"])
        cur.wait_stream(self.post_stream)
        return self.b["post"]
