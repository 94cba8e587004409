"""The multi-process scaffolding of the sharded tests, once: run_world() starts one process per rank of a torch.distributed/gloo world
and watches them; rank_main() is what every worker script (tests/_gloo_*worker*.py) does around its own computation.

What run_world() guarantees: no pipes (every rank logs to a file of its own, so no rank can block on output), one deadline for the whole
world, a rank that dies ends the world (its peers get GRACE_S seconds, then are killed) and is named first in the failure, and at most
MAX_WORLD ranks.  Nothing in the product imports this module."""
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

GRACE_S = 10          # what the peers of a dead rank get to exit on their own: they cannot pass their next collective, so any value well under
#                       the tests' timeouts serves
MAX_WORLD = 16        # processes that may hold one GPU open at the same time
POLL_S = 0.05
TAIL_LINES = 40


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _log_path(out, rank):
    return out + ".rank%d.log" % rank


def _tail(path):
    with open(path, errors="replace") as f:
        return "".join(f.readlines()[-TAIL_LINES:])


def _code(rc):
    try:
        return "%d (%s)" % (rc, signal.Signals(-rc).name) if rc < 0 else str(rc)
    except ValueError:
        return str(rc)


def run_world(worker, world, out, *, timeout, per_rank=False, env=None, grace=GRACE_S):
    """Run `worker` (a file name under tests/, or a full argv list) as `world` ranks over gloo on 127.0.0.1, each with the result path `out`
    as its last argument, its output in <out>.rank<r>.log.  Returns np.load(out), or with per_rank the list of np.load(<out>.rank<r>.npz).
    `timeout` seconds from the first start everything still running is killed; `grace` seconds after the first rank exits non-zero
    likewise.  Either way an AssertionError names the cause first."""
    assert world <= MAX_WORLD, "a world of %d: at most %d processes may hold the GPU open at the same time" % (world, MAX_WORLD)
    argv = ([sys.executable, os.path.join(HERE, worker)] if isinstance(worker, str) else list(worker)) + [out]
    port = free_port()
    procs, killed, first_bad = [], [], None
    try:
        deadline = time.monotonic() + timeout
        for r in range(world):
            rank_env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r))
            rank_env.update(env or {})
            with open(_log_path(out, r), "wb") as log:
                procs.append(subprocess.Popen(argv, env=rank_env, stdout=log, stderr=subprocess.STDOUT))
        kill_at = deadline
        while time.monotonic() < kill_at:
            codes = [p.poll() for p in procs]             # all of them, in no order: nobody is waited for
            if None not in codes:
                break
            if first_bad is None and any(codes):
                first_bad = next(r for r, c in enumerate(codes) if c)
                kill_at = min(deadline, time.monotonic() + grace)
            time.sleep(POLL_S)
    finally:
        for r, p in enumerate(procs):
            if p.poll() is None:
                p.kill()                      # exactly the processes started here
                p.wait()
                killed.append(r)
    if first_bad is None:
        first_bad = next((r for r, p in enumerate(procs) if p.returncode and r not in killed), None)
    if first_bad is not None or killed:
        if first_bad is not None:
            report = ["rank %d failed first: return code %s\n%s" % (first_bad, _code(procs[first_bad].returncode), _tail(_log_path(out, first_bad)))]
            why = "killed by the launcher after rank %d failed" % first_bad
        else:
            report = ["the world of %d timed out after %g s" % (world, timeout)]
            why = "timed out, killed by the launcher"
        for r, p in enumerate(procs):
            if r in killed:
                report.append("rank %d: %s\n%s" % (r, why, _tail(_log_path(out, r))))
            elif p.returncode and r != first_bad:
                report.append("rank %d: return code %s\n%s" % (r, _code(p.returncode), _tail(_log_path(out, r))))
        raise AssertionError("\n".join(report))
    return [np.load(out + ".rank%d.npz" % r) for r in range(world)] if per_rank else np.load(out)


def rank_main(body, *, gpu=False, per_rank=False):
    """One rank of a worker script: join the gloo world, call body(comm, ctx) and save the dict it returns (None: this rank saves nothing) to
    sys.argv[1], or with per_rank to <sys.argv[1]>.rank<r>.npz.  comm is backends.GlooComm and ctx None on the CPU; with gpu the rank opens
    its own context on GPU 0 and comm is backends.HostStagedComm on it."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="env://")
    from backends import GlooComm, HostStagedComm
    ctx = None
    if gpu:
        from tomography_alignment_amd import _lib
        ctx = _lib.Context(0)
    comm = HostStagedComm(ctx) if gpu else GlooComm()
    out = body(comm, ctx)
    if out is not None:
        np.savez(sys.argv[1] + (".rank%d.npz" % comm.rank if per_rank else ""), **out)
    dist.barrier()
    if ctx is not None:
        ctx.close()
    dist.destroy_process_group()
