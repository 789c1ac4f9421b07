"""The rank launcher of the data-parallel tests: ``world`` spawned processes over gloo on one machine."""
import socket


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker, world, *args, results=1, get_timeout=600, ranks=None):
    """Starts ``worker(rank, world, port, *args, queue)`` for every rank (``ranks``: only those) in a spawn context,
    takes ``results`` items off the queue (``get_timeout`` seconds each), joins the workers and requires exit code 0
    of each.  Returns the items in the order they arrived.  ``worker`` is a top-level function of its test module:
    spawn pickles it by module path."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ranks = range(world) if ranks is None else ranks
    procs = [ctx.Process(target=worker, args=(r, world, port, *args, q)) for r in ranks]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=get_timeout) for _ in range(results)]
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    codes = [p.exitcode for p in procs]
    assert all(c == 0 for c in codes), f"{worker.__name__}: exit codes {codes}"
    return got
