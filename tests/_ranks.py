"""Runs a worker function as `world` spawned ranks and collects one result per
rank (shared by the multi-process tests; imported, not a conftest).

The ranks meet through a file:// rendezvous in a fresh temporary directory:
a port probed as free and handed to the workers can be taken by another
process before rank 0 binds it.  A rank that dies fails the test at once
instead of after the queue's time limit, and no rank outlives the test (a
rank left waiting for a peer that died would keep the interpreter from
exiting)."""
import queue
import shutil
import tempfile
import time


def run_ranks(target, world, make_args, timeout=300, join_timeout=120):
    """target(*make_args(rank, rdv, q)) per rank, where rdv is the init_method
    for dist.init_process_group and q the queue each rank puts one result on;
    returns the `world` results in arrival order."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tmp = tempfile.mkdtemp(prefix="rram_rdv_")
    ps = [ctx.Process(target=target, args=make_args(r, f"file://{tmp}/rdv", q)) for r in range(world)]
    try:
        for p in ps:
            p.start()
        res, deadline = [], time.monotonic() + timeout
        while len(res) < world:
            try:
                res.append(q.get(timeout=1.0))
            except queue.Empty:
                dead = [(i, p.exitcode) for i, p in enumerate(ps) if p.exitcode not in (None, 0)]
                assert not dead, f"rank(s) died before reporting: (rank, exit code) {dead}"
                assert time.monotonic() < deadline, f"{world - len(res)} of {world} ranks did not report in {timeout} s"
        for i, p in enumerate(ps):
            p.join(timeout=join_timeout)
            assert p.exitcode == 0, (i, p.exitcode)
        return res
    finally:
        for p in ps:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
        shutil.rmtree(tmp, ignore_errors=True)
