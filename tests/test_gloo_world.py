"""tests/gloo_world.py::run_world itself, on the CPU with tiny `-c` ranks: both result forms, a rank that prints more than a pipe holds, a
rank that dies (the world ends within the grace period and the dead rank is named first), one deadline for the whole world, the size cap."""
import os
import subprocess
import sys
import time

import pytest

import gloo_world
from gloo_world import run_world

INIT = "import sys, time, numpy as np, torch.distributed as dist; dist.init_process_group('gloo', init_method='env://'); r = dist.get_rank()\n"


def _rank(code):
    return [sys.executable, "-c", code]


@pytest.fixture
def started(monkeypatch):
    """The Popen objects run_world creates."""
    procs, real = [], subprocess.Popen

    def popen(*a, **kw):
        procs.append(real(*a, **kw))
        return procs[-1]
    monkeypatch.setattr(subprocess, "Popen", popen)
    return procs


def test_passing_world_returns_both_result_forms(tmp_path):
    out = str(tmp_path / "p")
    ranks = run_world(_rank(INIT + "np.savez(sys.argv[1] + '.rank%d.npz' % r, rank=r); dist.barrier()"), 2, out, timeout=60, grace=2, per_rank=True)
    assert [int(w["rank"]) for w in ranks] == [0, 1]
    out = str(tmp_path / "one.npz")
    got = run_world(_rank(INIT + "r == 0 and np.savez(sys.argv[1], rank=r, world=dist.get_world_size()); dist.barrier()"), 2, out, timeout=60, grace=2)
    assert int(got["rank"]) == 0 and int(got["world"]) == 2
    assert sorted(os.listdir(str(tmp_path))) == ["one.npz", "one.npz.rank0.log", "one.npz.rank1.log", "p.rank0.log", "p.rank0.npz", "p.rank1.log", "p.rank1.npz"]


def test_environment_is_the_callers_plus_the_rendezvous(tmp_path, monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    monkeypatch.setenv("OMP_NUM_THREADS", "16")
    code = ("import os, sys, numpy as np\n"
            "np.savez(sys.argv[1] + '.rank%s.npz' % os.environ['RANK'], **{k: os.environ[k] for k in "
            "('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'GPU_MAX_HW_QUEUES', 'OMP_NUM_THREADS')})")
    a = run_world(_rank(code), 2, str(tmp_path / "a"), timeout=60, grace=2, per_rank=True)
    b = run_world(_rank(code), 1, str(tmp_path / "b"), timeout=60, grace=2, per_rank=True, env={"OMP_NUM_THREADS": "1"})
    for r, w in enumerate(a):
        assert (str(w["RANK"]), str(w["LOCAL_RANK"]), str(w["WORLD_SIZE"]), str(w["MASTER_ADDR"])) == (str(r), str(r), "2", "127.0.0.1")
        assert str(w["MASTER_PORT"]) == str(a[0]["MASTER_PORT"]) and str(w["GPU_MAX_HW_QUEUES"]) == "4" and str(w["OMP_NUM_THREADS"]) == "16"
    assert str(b[0]["OMP_NUM_THREADS"]) == "1" and str(b[0]["GPU_MAX_HW_QUEUES"]) == "4"


def test_a_chatty_rank_does_not_block_the_world(tmp_path):
    """Rank 1 prints 1 MiB -- many times what a pipe holds -- before the barrier rank 0 waits in.  With one pipe per rank drained in rank
    order this world sat until its timeout."""
    out = str(tmp_path / "c.npz")
    code = INIT + "r == 1 and sys.stdout.write('x' * (1 << 20)); sys.stdout.flush(); dist.barrier(); r == 0 and np.savez(sys.argv[1], ok=1)"
    t0 = time.monotonic()
    got = run_world(_rank(code), 2, out, timeout=60, grace=2)
    assert int(got["ok"]) == 1 and time.monotonic() - t0 < 30
    assert os.path.getsize(out + ".rank1.log") >= 1 << 20


def test_a_dead_rank_ends_the_world_and_is_named_first(tmp_path, started):
    code = INIT + "r == 1 and (print('MARKER rank 1 gives up', flush=True), sys.exit(3)); time.sleep(60)"
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_world(_rank(code), 2, str(tmp_path / "d.npz"), timeout=60, grace=2)
    assert time.monotonic() - t0 < 2 + 15                  # grace + starting two interpreters that import torch, not rank 0's 60 s
    msg = str(e.value)
    first, rest = msg.split("rank 0", 1)
    assert first.startswith("rank 1 failed first: return code 3\n") and "MARKER rank 1 gives up" in first
    assert rest.startswith(": killed by the launcher")
    assert len(started) == 2 and all(p.poll() is not None for p in started)
    assert started[0].returncode < 0 and started[1].returncode == 3


def test_a_signal_is_printed_by_name(tmp_path, started):
    """A rank that ends on a signal (here one it sends itself: nothing faults) is reported with the signal's name."""
    code = "import os, signal; os.environ['RANK'] == '0' and os.kill(os.getpid(), signal.SIGTERM)"
    with pytest.raises(AssertionError) as e:
        run_world(_rank(code), 2, str(tmp_path / "s.npz"), timeout=60, grace=2)
    assert str(e.value).startswith("rank 0 failed first: return code -15 (SIGTERM)")
    assert all(p.poll() is not None for p in started)


def test_one_deadline_for_the_world(tmp_path, started):
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        run_world(_rank("import time; time.sleep(60)"), 3, str(tmp_path / "t.npz"), timeout=3, grace=2)
    assert 3 <= time.monotonic() - t0 < 3 + 2 + 5          # one deadline, not one per rank
    msg = str(e.value)
    assert msg.startswith("the world of 3 timed out after 3 s")
    assert all("rank %d: timed out, killed by the launcher" % r in msg for r in range(3))
    assert len(started) == 3 and all(p.poll() is not None for p in started)


def test_world_above_16_is_refused_before_anything_starts(tmp_path, started, monkeypatch):
    ports = []
    monkeypatch.setattr(gloo_world, "free_port", lambda: ports.append(1) or 1)
    with pytest.raises(AssertionError):
        run_world(_rank("pass"), 17, str(tmp_path / "big.npz"), timeout=20, grace=2)
    assert not started and not ports and os.listdir(str(tmp_path)) == []
