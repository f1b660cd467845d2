"""What has to happen around a hipGraph capture, once, for every graph holder of the package (rollout.GraphedRollout /
GraphedTrigger / GraphedSampler, train_graphs.GraphedIteration / SegmentedIteration, benchlib's layer timings):

1. the eager warm-up runs on the process-wide warm-up stream and the capturing stream waits for it (`warm_up`);
2. the skip-dependent caches are emptied before a group of captures - a graph must not read what an eager call cached - and
   after it - eager code must not read what lives in a graph's private pool (`skip_scope`);
3. the capture uses the thread-local error mode (`CAPTURE_KW`, `capturing`);
4. right after the capture the holder takes `snapshot_eager_caches()` and keeps it as long as the graph lives (`capture`);
5. a capture that raises drops every version-keyed cache and the deferred weight-gradient queues (`capturing`);
6. a graph that STEPS parameters (train_graphs) builds every parameter-derived tensor itself: what an eager call derived from
   the current parameter version is forgotten before the capture (`drop_parameter_forms`).  Inside the capture a form is
   rebuilt after every optimiser step because `FusedAdam.step` advances the parameters' version counters while capturing too.

Host only: no kernel is launched from here."""
from __future__ import annotations

import contextlib

import torch

from . import _derived

# Streams are made ONCE per process and shared by every graph holder of the package.  torch hands out streams from a pool of 32
# per device, round-robin and without telling: a process that builds many samplers (bench.py: two families x (three chains +
# make_gifs) + C1) wraps around the pool, after which two "concurrent" chains may sit on ONE hip stream (silently serial), or a
# chain's stream may be the one torch captures graphs on - the r06 bench died with a segmentation fault inside
# hipGraphLaunch (hip::Graph::UpdateStreams) at exactly that point.  Work on one stream runs in order, so sharing the streams
# between holders is safe; it only orders work that a caller issues from different holders at the same time.
_streams = {}


def pooled_stream(role: str, index: int = 0) -> "torch.cuda.Stream":
    key = (torch.cuda.current_device(), role, index)
    if key not in _streams:
        _streams[key] = torch.cuda.Stream()
    return _streams[key]


# Graph captures use the thread-local error mode: what OTHER threads do while this thread captures (torch.distributed's
# watchdog polling the events of earlier collectives when a process group exists) is none of the capture's business; the
# autograd engine's worker threads still launch into the capturing stream.
CAPTURE_KW = {"capture_error_mode": "thread_local"}


def drop_version_keyed_caches() -> None:
    """Forget every tensor the module-level caches hold - every cache registered with _derived: packed / transposed /
    Winograd-domain weights, BatchNorm folds, embed-folded cell weights, GEMM-operand forms, hoisted skip halves and
    projections, device index maps and loss weights, split-K workspaces, the LSTM's shared zero state.  For the one
    situation in which an entry can be WRONG although its key matches: a hipGraph capture that raised part-way.
    During a capture a cache miss allocates from the graph's private pool and records the kernels that
    would fill the tensor - nothing executes - and the entry is stored under the current parameter version; when the
    capture is abandoned the pool is freed, but the entry would still be hit by the next eager call, which would read
    never-written (and freed) memory.  Everything here is rebuilt on demand from the parameters.
    The deferred weight-gradient queues go with them: a capture that dies INSIDE backward() skips autograd's
    end-of-backward callback, so operands queued during it - pointers into the freed pool, never written - would be
    flushed into .grad by the next eager backward (or block its flush: the `flush queued` flag stays set)."""
    from . import autograd as ag
    ag.drop_deferred_wgrads()
    _derived.drop_all()


def drop_parameter_forms() -> None:
    """Forget the tensors derived from parameters (packed / transposed / Winograd-domain weights, GEMM-operand forms, folds)
    before the capture of a graph that steps those parameters.  A form is built once per parameter version whoever asks, so
    the closure that opens a training iteration finds the forms that the last closure of the previous iteration built from
    the same version; captured, it would record no build and every replay would read the weights of the eager warm-up.
    After this, each form's build is recorded in the graph ahead of its first use."""
    _derived.drop_derived()


def snapshot_eager_caches() -> list:
    """Strong references to every tensor the module-level caches hold right now - every cache registered with _derived: the
    LSTM's shared zero state, packed / transposed / Winograd-domain weights, BatchNorm folds, the embed-folded first-cell
    weights, GEMM-operand forms of the dense ends, skip halves and projections, device index maps and loss weights.
    A captured hipGraph reads such tensors by RAW POINTER when they were created eagerly during its warm-up;
    the caches drop entries with their owner or past a size bound, and replace them when a parameter version changes
    (load_state_dict, an optimiser step), after which the allocator may hand the block to someone else while live graphs
    still read it.  Every graph holder keeps the snapshot taken right after its capture for as long as it lives."""
    from . import ops
    if not torch.cuda.is_current_stream_capturing():
        # the capture that just ended no longer needs its split-K workspace OBJECTS (and the snapshot must not pin them)
        ops.evict_captured_workspaces()
    return _derived.snapshot()


def warm_up(fn, times: int = 1):
    """fn() `times` times on the warm-up stream, the current stream waiting for it: first-launch work (weight packs, LDS
    attributes, BN folds) must not be captured.  Returns fn's last result."""
    side = pooled_stream("warmup")
    side.wait_stream(torch.cuda.current_stream())
    out = None
    with torch.cuda.stream(side):
        for _ in range(times):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return out


@contextlib.contextmanager
def capturing(pool=None):
    """A new graph that records what its body launches (thread-local error mode; `pool`: share another graph's private
    pool).  A body - or the end of the capture - that raises leaves cache entries and queued weight gradients that point into
    the abandoned pool and were never written: they are dropped (drop_version_keyed_caches) before the exception goes on."""
    graph = torch.cuda.CUDAGraph()
    kw = CAPTURE_KW if pool is None else dict(CAPTURE_KW, pool=pool)
    try:
        with torch.cuda.graph(graph, **kw):
            yield graph
    except BaseException:
        drop_version_keyed_caches()
        raise


def capture(fn, pool=None) -> tuple:
    """(graph, fn's result, keepalive): fn() recorded into a new graph, and the eager tensors the graph reads by raw pointer,
    to be kept for as long as it lives."""
    with capturing(pool) as graph:
        out = fn()
    return graph, out, snapshot_eager_caches()


class skip_scope:
    """The skip-dependent caches (hoisted skip halves, skip projections) around a group of captures: empty on entry -
    nothing cached eagerly may be referenced by a graph - and on exit - nothing from a graph's pool by later eager calls.
    In between the entries stay, so that a later graph of the group reads the buffers an earlier one writes; `mark()` /
    `drop_since(mark)` forget what one capture added where the next must not see it."""
    mark = staticmethod(_derived.skip_mark)
    drop_since = staticmethod(_derived.skip_drop_since)

    def __enter__(self):
        from . import fused, ops
        ops.clear_skip_proj_cache()
        fused.clear_skip_hoist_cache()
        return self

    def __exit__(self, *exc):
        self.__enter__()
