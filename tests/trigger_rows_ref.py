"""The per-row variance trigger's reference (no GPU, no project code): seeded input sets and the reference's own arithmetic -
generate_frames.py:231 (`np.concatenate([context_array[1:], [value]])`) and :288-289 (`np.mean + coef * np.std`, `value >
threshold`) in numpy float32 - applied to every batch row by itself, with the rule's bookkeeping around it
(docs/DESIGN_NOTES_trigger_rows.md): the first W values fill the window, a decision is taken at the prediction steps whose value
slid a full window, a row draws again only more than `gap` steps after its last draw."""
import numpy as np

# (D, B, W, T): the kernel cases.  130 latent dims = three strides of the wave with a ragged end, W = 5 where coef 2.01 can never
# draw; W = 64, the widest window, every lane a window element; the 1 x 1 x 1 corner; the reference's 90 x 50 x 12.
CASES = [(130, 3, 5, 20), (64, 7, 64, 70), (1, 1, 1, 6), (90, 50, 12, 30)]
SEEDS = {(130, 3, 5, 20): 0, (64, 7, 64, 70): 1, (1, 1, 1, 6): 2, (90, 50, 12, 30): 0}
COEFS = (2.01, -0.5)
GAPS = (0, 3)
GUARD = 1e-4         # trigger_window_decide's comment: device and numpy may decide differently only inside this relative margin


def n_pasts(case):
    """n_past = 2 everywhere; the W = 64 case also with W + 3: its window slides during the conditioning steps."""
    return (2, case[2] + 3) if case == CASES[1] else (2,)


def case(D, B, W, T, seed):
    """var (T, D, B) float32 - var[i] is the predictive variance of step i, var[0] unused - and values (T, B) float32, the rows'
    norms.  Lognormal variances; 15 % of the (step, row) entries three times as large: the spikes the rule is there to find."""
    rng = np.random.RandomState(1000 + seed)
    var = rng.lognormal(-3.0, 0.3, (T, D, B)).astype(np.float32)
    spikes = rng.random_sample((T, B)) < 0.15
    var = (var * np.where(spikes, 3.0, 1.0)[:, None, :]).astype(np.float32)
    values = np.linalg.norm(var.transpose(0, 2, 1), axis=2).astype(np.float32)
    return var, values


def decide(values, n_past, W, coef, gap, device_flags=None, guard=GUARD):
    """values (T, B) float32, row 0 unused -> (flags (T, B) int32, thresholds (T, B) float32 with +inf where no decision is taken,
    margins (T, B) float64 with nan there, windows (B, W) after the last step).
    device_flags (T, B): a decision whose margin is inside `guard` takes the device's flag for the gap bookkeeping (and for the
    returned flag); the caller counts them from the margins."""
    T, B = values.shape
    flags = np.zeros((T, B), dtype=np.int32)
    thresholds = np.full((T, B), np.inf, dtype=np.float32)
    margins = np.full((T, B), np.nan)
    windows = np.zeros((B, W), dtype=np.float32)
    for b in range(B):
        context_array = np.zeros(0, dtype=np.float32)
        last = None
        for i in range(1, T):
            value = values[i, b]
            if len(context_array) < W:
                context_array = np.concatenate([context_array, [value]])
                continue
            context_array = np.concatenate([context_array[1:], [value]])                 # :231
            if i < n_past:
                continue
            threshold = np.mean(context_array) + coef * np.std(context_array)            # :288
            draw = bool(value > threshold)                                               # :289
            margins[i, b] = abs(float(value) - float(threshold)) / abs(float(threshold))
            draw = draw and (last is None or i - last > gap)
            if device_flags is not None and margins[i, b] <= guard:
                draw = bool(device_flags[i, b])
            if draw:
                last = i
            flags[i, b], thresholds[i, b] = int(draw), threshold
        windows[b, :len(context_array)] = context_array
    return flags, thresholds, margins, windows
