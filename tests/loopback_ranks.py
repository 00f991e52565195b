"""Imported by the WORKERS of the two-rank loopback tests (loopback_util.py runs them): the two ranks are two threads of the worker's
process, each with its own context on device 0 and a communicator of a world of two."""
import threading

from immutable3_amd import native

WORLD = 2


def both(fn):
    """Run fn(rank) on two threads (the two ranks); returns their results and what they raised."""
    out, err = [None] * WORLD, [None] * WORLD

    def run(r):
        try:
            out[r] = fn(r)
        except BaseException as e:      # noqa: BLE001
            err[r] = e
    ts = [threading.Thread(target=run, args=(r,)) for r in range(WORLD)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "a rank is stuck in a collective: the ranks did not take the same exit"
    return out, err


def start():
    """(contexts, communicators) of the two ranks; the communicators are created on the ranks' own threads, as RCCL wants them."""
    ctxs = [native.Context(0) for _ in range(WORLD)]
    uid = native.comm_unique_id()
    comms = [None] * WORLD

    def mk(r):
        comms[r] = native.Comm(ctxs[r], WORLD, r, uid)
    out, err = both(mk)
    assert err == [None, None], err
    return ctxs, comms
