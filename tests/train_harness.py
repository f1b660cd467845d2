"""What the GPU tests of the Trainer share: the smallest options the closures accept (dcgan_64, batch 4, n_past 2, n_future 2,
the in-repo synthetic smmnist), a seeded Trainer, its batches, a loop over iterations eager or as a GraphedIteration, and
train.py as a child process with one rank or several.  A plain module (`from tests import train_harness`), not a conftest."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ARGS = ["--model", "dcgan", "--batch_size", "4", "--n_past", "2", "--n_future", "2", "--n_eval", "4", "--dataset", "smmnist"]
RENDEZVOUS = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
# the rehearsal switches of tests/test_gpu_multirank.py: every rank on GPU 0, collectives over gloo
REHEARSAL = {"DVG_DP_SHARE_GPU": "1", "DVG_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "2"}


def opt(extra=(), model="dcgan"):
    import train
    return train.options(ARGS + ["--model", model, "--niter", "1", "--epoch_size", "1", "--no_save"] + list(extra))


def trainer(extra=(), seed=3, model="dcgan"):
    import train
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    tr = train.Trainer(opt(extra, model), torch.device(DEV))
    tr.train_mode()
    return tr


def make_batches(n, seq_len=4, seed=9, batch=4):
    import utils
    from dvg_amd.data import SyntheticMovingMNIST
    gen = SyntheticMovingMNIST(seq_len=seq_len, seed=seed)
    return [utils.normalize_data(opt(), torch.cuda.FloatTensor, gen.batch(batch))[0] for _ in range(n)]


def arena(tr):
    return {n: getattr(tr.arena, n).clone() for n in ("p", "m", "v")}


def iterate(tr, xs, graphed=False, warmup=1, each=None):
    """The iterations over xs, eager or as GraphedIteration(warmup).  Returns (step, [(what the iteration returned, what
    each(tr, step, i) returned after it), ...]); a graphed step must not have fallen back to eager iterations."""
    import train
    step = train.GraphedIteration(tr, warmup=warmup) if graphed else tr.iteration
    torch.manual_seed(77)                    # the GP samples of the iterations
    out = []
    for i, x in enumerate(xs):
        res = step(x)
        out.append((res, each(tr, step, i) if each is not None else None))
    torch.cuda.synchronize()
    if graphed:
        assert not step.failed and step.graph is not None
    return step, out


def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def clean_env(**extra):
    """The environment without a launcher's rendezvous variables (a child that starts its own launcher, or none), plus `extra`."""
    env = {k: v for k, v in os.environ.items() if k not in RENDEZVOUS}
    env.update(extra)
    return env


def launcher(ranks):
    """The interpreter's arguments in front of a script: nothing for one rank, `torch.distributed.run` on a free port for several."""
    return [] if ranks == 1 else ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr",
                                  "127.0.0.1", "--master-port", str(free_port())]


def run_train_py(args, ranks=1, env=None, timeout=600):
    """train.py as a fresh child process per rank; env: variables on top of clean_env().  Returns the CompletedProcess."""
    return subprocess.run([sys.executable] + launcher(ranks) + [os.path.join(ROOT, "train.py")] + list(args), cwd=ROOT,
                          env=clean_env(**(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
