"""How train.py replays its iterations: one hipGraph per iteration (GraphedIteration), a chain of hipGraphs cut at the gradient
all-reduces for several ranks (SegmentedIteration), and the background thread that draws the next batch while the GPU works
(BatchPrefetcher).  Re-exported by train.py (`train.GraphedIteration` etc.); the closures, the iteration body that is captured
here (Trainer._iteration_dev) and the Trainer state they drive are in dvg_amd/trainer.py."""
import sys

import torch

from . import fused, graphs


class GraphedIteration:
    """`Trainer.iteration` as ONE hipGraph (torch.cuda.CUDAGraph): forward, the three backward passes, the gradient
    all-reduces and the four fused Adam steps - several thousand launches whose Python + ctypes cost otherwise bounds
    the small per-GPU batches of the data-parallel configs (dcgan_64 at 16 / GPU: 41 ms of kernels in a 132 ms
    iteration).  The first `warmup` calls run eagerly (they are ordinary training steps: weight packs, LDS attributes,
    GP prior initialisation and allocator warm-up happen there); the next call captures and replays; later calls replay.
    After each replay the version counters of all parameters and buffers are bumped (the graph writes them through raw
    pointers; the packed-weight / BN-fold caches key on versions) and the optimisers' host-side step counts advance.
    A change of any learning rate (MultiStepLR, train.py:105-106) triggers a re-capture - `--lr_schedule` changes none: its multiplier
    lives on the device (dvg_amd/lr_schedule.py) -, and so does Trainer.load_state_dict
    (the device-side Adam step counts are seeded from the restored host counts by begin_capture)."""

    def __init__(self, trainer, warmup: int = 2):
        self.tr, self.warmup = trainer, warmup
        self.calls = 0
        self.graph = None
        self.sig = None
        self.failed = False          # a capture raised: eager iterations from then on
        self.outs = self._keepalive = None

    def _replay(self):
        self.graph.replay()

    def _signature(self, x):
        lrs = tuple(g['lr'] for o in self.tr.optimizers() for g in o.param_groups)
        return (lrs, tuple(tuple(t.shape) for t in x), self.tr.opt.ft, tuple(m.training for m in self.tr.modules),
                self.tr.state_loads)     # Trainer.load_state_dict: another state behind the same pointers

    def _release(self):
        """Drop the captured graph(s) and everything they keep alive BEFORE a re-capture allocates a new private pool
        (a MultiStepLR milestone re-captures: two pools of 12-17 GB of saved Winograd transforms need not coexist)."""
        self.graph = None
        self.outs = None
        self._keepalive = None
        torch.cuda.synchronize()

    def _capture(self, x):
        tr = self.tr
        self._release()
        self.static_x = [t.clone() for t in x]
        for o in tr.optimizers():
            o.begin_capture()
        torch.cuda.synchronize()
        graphs.drop_parameter_forms()                # every replay re-derives the weight forms from the stepped parameters
        self._record()
        for o in tr.optimizers():
            o.end_capture()                          # every group a captured zero_grads() ticked was stepped in the capture
        self._keepalive = graphs.snapshot_eager_caches()    # eager tensors the graph reads by raw pointer stay alive with it
        self.sig = self._signature(x)

    def _record(self):
        with graphs.capturing() as self.graph:
            self._body()

    def _body(self):
        self.outs = self.tr._iteration_dev(self.static_x)   # the eager iteration's launches: schedule tick first, EMA update last

    def __call__(self, x):
        tr = self.tr
        self.calls += 1
        if self.calls <= self.warmup or self.failed or fused.sync_bn_world() > 1:   # sync-BN: collectives inside every pass
            return tr.iteration(x)
        if self.graph is None or self.sig != self._signature(x):
            try:
                self._capture(x)
            except Exception as e:   # noqa: BLE001 - out of memory for the pool, a partially used Adam group, ...
                # A capture executes nothing: parameters, moments and BatchNorm statistics are untouched.  Fall back to the
                # eager iteration for the rest of the run (no re-exec, no retry: the same capture would fail again).
                self.failed = True
                self._release()
                for o in tr.optimizers():
                    o._captured_groups = []
                tr._segmenter = None
                # ... except the module-level caches: a miss DURING the capture stored a tensor from the graph's pool whose
                # fill was recorded, never run, under the current parameter version.  The eager iteration below must not
                # hit those entries (never-written, freed memory): drop every version-keyed cache, rebuilt on demand.
                graphs.drop_version_keyed_caches()
                tr._ft_cache = None
                tr.frame_predictor.hidden = None
                print(f"train: hipGraph capture failed ({type(e).__name__}: {str(e)[:200]}); continuing with eager "
                      "iterations", file=sys.stderr, flush=True)
                return tr.iteration(x)
        for o in tr.optimizers():
            o.check_graph_fresh()        # an eager step() since the capture left the device-side Adam step counts behind
        for dst, src in zip(self.static_x, x):
            dst.copy_(src)
        self._replay()
        for o in tr.optimizers():
            o.after_graph_replay()
        with torch.no_grad():
            for m in tr.modules:
                for b in m.buffers():
                    torch.autograd.graph.increment_version(b)   # BatchNorm running statistics
        return tr._iteration_result(self.outs)


class SegmentedIteration(GraphedIteration):
    """The data-parallel form of GraphedIteration: the iteration is captured as a CHAIN of hipGraphs cut at the gradient
    all-reduces, which run eagerly between the segments (train_model: [forward + decoder / LSTM / GP backward] -> start
    all-reduce of their ranges -> [encoder backward] -> start the encoder range, wait for both -> [four Adam steps +
    LSTM closure] -> all-reduce -> [LSTM Adam + GP closure] -> all-reduce -> [GP Adam]).  No collective is ever inside a
    captured graph - RCCL runs them on its own stream exactly as in the eager loop, overlap with the encoder phase
    included - and the ≈2 500 launches of an iteration still replay without Python.  All segments share one memory pool
    and are always replayed in capture order."""

    def _release(self):
        self.items, self._pool, self._cur, self._ctx = [], None, None, None
        super()._release()

    def _record(self):
        tr = self.tr
        tr._segmenter = self
        try:
            self._begin()
            self._body()
            self._end()
        except BaseException:
            if self._ctx is not None:          # a segment is still being captured: end the capture before unwinding
                ctx, self._ctx, self._cur = self._ctx, None, None
                try:
                    ctx.__exit__(*sys.exc_info())
                except Exception:   # noqa: BLE001 - the original exception is the one to report
                    pass
            raise
        finally:
            tr._segmenter = None
        self.graph = [g for kind, g in self.items if kind == "graph"]   # (truthy: "captured"; replay goes through items)

    def _begin(self):
        self._ctx = graphs.capturing(self._pool)
        self._cur = self._ctx.__enter__()

    def _end(self):
        self._ctx.__exit__(None, None, None)
        if self._pool is None:
            self._pool = self._cur.pool()
        self.items.append(("graph", self._cur))
        self._cur = self._ctx = None

    def cut(self, actions):
        self._end()
        self.items.append(("eager", actions))
        self._begin()

    def _replay(self):
        for kind, item in self.items:
            if kind == "graph":
                item.replay()
            else:
                self.tr._run_ar(item)

    @property
    def n_segments(self):
        return sum(1 for k, _ in self.items if k == "graph")


class BatchPrefetcher:
    """The host half of the input pipeline on a background thread, `depth` batches ahead.  A training iteration ends with
    the host waiting for the GPU (the closures' loss values are read back like train.py:361-362 does); drawing the next
    batch only then left the GPU idle for the whole host-side generation (19 ms of a 102 ms dcgan_64 iteration).  The
    thread runs while the main thread waits (the wait releases the GIL); batches come out in the generator's order."""

    def __init__(self, gen, depth=2):
        self.gen, self.depth = gen, depth
        # where the CONSUMER stands: the position carried by the last batch handed out (data.BatchStream), not the generator's,
        # which is up to `depth` + 1 batches further on
        self._pos = gen.position() if hasattr(gen, "position") else None
        self._start()

    def _start(self):
        import queue
        import threading
        self.q, self._stop = queue.Queue(self.depth), threading.Event()
        self.thread = threading.Thread(target=self._run, args=(self.q, self._stop), daemon=True)
        self.thread.start()

    _END = object()

    def _run(self, q, stop):
        try:
            for item in self.gen:
                q.put(item)
                if stop.is_set():
                    return
            q.put(self._END)
        except BaseException as e:   # noqa: BLE001 - handed to the consumer
            q.put(e)

    def position(self):
        """The data position after the batches consumed so far (None in front of a generator that has none)."""
        return self._pos

    def restore(self, pos):
        """Continue from `pos`: the thread is stopped (whatever it drew ahead is dropped), the generator restored, and a new
        thread started.  The next batch is the one that followed `pos` in the run that saved it."""
        import queue
        self._stop.set()
        while self.thread.is_alive():          # blocked in put(), or about to put: make room until it has seen the flag
            try:
                while True:
                    self.q.get_nowait()
            except queue.Empty:
                pass
            self.thread.join(0.002)
        self.gen.restore(pos)
        self._pos = self.gen.position()
        self._start()

    def __iter__(self):
        return self

    def __next__(self):
        item = self.q.get()
        if item is self._END:
            self.q.put(item)         # stay exhausted
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        self._pos = getattr(item, "position", self._pos)
        return item
