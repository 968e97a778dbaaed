"""Helpers of the stream-ordering tests (tests/test_gpu_streams_*.py): no tests here.

The technique is that of tests/test_gpu_offgrid.py::test_copy_bytes_runs_on_the_current_stream.  The stream a product call is
made on is kept busy by a bounded spin, the call's inputs are rewritten on that stream BEHIND the spin, and only then is the call
made.  Work the product orders correctly runs behind the rewrite and sees the new inputs; work it puts on another stream, or fails
to order behind the caller's stream, runs while the spin is still going and reads the bytes the buffers held before.  With kernels
that are reproducible bit for bit, a missing dependency is then a bitwise mismatch, not a rare race.

What makes such a test prove something is the precondition ``enqueued_behind``: when the product call returned to the host, the
spin had not finished, so everything the call enqueued was enqueued while its stream was busy.  A test that cannot establish it
fails; it never passes without it.
"""
import time

import torch

MIN_STALL_MS, MAX_STALL_MS = 20.0, 250.0


def calibrate():
    """Spin cycles of ``torch.cuda._sleep`` per millisecond on this device: two timing events around a spin, the median of
    three.  Printed, and measured once per test module (a module-scoped fixture calls this)."""
    n = 20_000_000
    torch.cuda._sleep(1000)                               # (loads the spin kernel)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    per_ms = n / sorted(ms)[1]
    print(f"stream harness: torch.cuda._sleep runs {per_ms:.0f} cycles per millisecond ({n} cycles took {sorted(ms)[1]:.2f} ms)")
    return per_ms


def stall_ms(host_seconds):
    """The stall for a call whose unstalled warm-up took ``host_seconds`` on the host: four times that, at least 20 ms, at most
    250 ms.  Whether it was enough is decided by ``enqueued_behind``, not here."""
    return min(MAX_STALL_MS, max(MIN_STALL_MS, 4.0e3 * host_seconds))


def stall(stream, ms, cycles_per_ms):
    """A bounded spin of ``ms`` milliseconds enqueued on ``stream`` -> the stall-end event, recorded right behind it."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms))
        end = torch.cuda.Event()
        end.record(stream)
    return end


def enqueued_behind(stall_end):
    """True if the stall is still running: to be evaluated immediately after the product call returns."""
    return not stall_end.query()


def timed(fn):
    """-> (fn(), host seconds it took): for the unstalled warm-up of a call."""
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def as_bits(t):
    """A tensor as integers of its own width (NaN-safe equality, and a dtype ``torch.equal`` supports on every build)."""
    t = t.contiguous()
    if t.dtype == torch.uint16:
        return t.view(torch.int16)
    if t.dtype in (torch.float32,):
        return t.view(torch.int32)
    if t.dtype == torch.float16:
        return t.view(torch.int16)
    return t


def bits_equal(a, b):
    """a and b hold the same bits (shape and dtype included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(as_bits(a), as_bits(b.to(a.device)))


def host_copies(tensors):
    """Device tensors -> CPU clones (None stays None).  The copies run on the current stream: call this only once the event behind
    the producers has completed."""
    return [None if t is None else as_bits(t).cpu().clone() for t in tensors]


# ---- what the harness can see ---------------------------------------------------------------------------------------------------------
# A process has a handful of hardware queues, and streams that share one are ordered by the queue: work that a product bug puts on
# stream B cannot run ahead of a spin on stream A if both sit on one queue, and the test passes although the dependency is missing.
# So a stream that a test stalls is first PROBED with a planted bug -- a copy made on another stream in front of the rewrite of its
# source -- against the streams a wrong launch would land on, and only streams on which the planted bug is seen are used.

def planted_bug_is_seen(stalled, other, cycles_per_ms, copy=None, n=4099):
    """Steps 1-4 on a toy producer that copies under ``torch.cuda.stream(other)`` instead of on the current stream, ``stalled``
    (only valid bytes move; copy(src, dst): the copy, default ``dst.copy_(src)``) -> True if the harness reports the mismatch, i.e. the
    copy ran while ``stalled`` was still spinning and moved the bytes the source held before.  False: the two streams are serialised
    (one hardware queue), or the spin had ended."""
    g = torch.Generator().manual_seed(n)
    stale, fresh = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    copy = copy or (lambda src, dst: dst.copy_(src, non_blocking=True))
    torch.cuda.synchronize()
    with torch.cuda.stream(stalled):
        src = stale.clone()
        dst = torch.zeros_like(src)
    torch.cuda.synchronize()
    end = stall(stalled, MIN_STALL_MS, cycles_per_ms)
    with torch.cuda.stream(stalled):
        src.copy_(fresh, non_blocking=True)
        with torch.cuda.stream(other):                       # the planted bug: not the stream the caller is on
            copy(src, dst)
        behind = enqueued_behind(end)
        snap = dst.clone()
        done = torch.cuda.Event()
        done.record(stalled)
    done.synchronize()
    other.synchronize()                                      # (the planted copy itself: it ran on `other`)
    seen = behind and bits_equal(dst, stale) and bits_equal(snap, stale) and not bits_equal(dst, fresh)
    torch.cuda.synchronize()
    return bool(seen)


def visible_stream(cycles_per_ms, against=()):
    """A new stream on which the planted bug is seen against the null stream (where a launcher that ignores its stream argument
    lands), against a further new stream, and against every stream of ``against``.  Streams that fail the probe are passed over; the
    call fails if eight candidates in a row do: the harness would then be blind in this process."""
    passed_over = []
    for _ in range(8):
        s, other = torch.cuda.Stream(), torch.cuda.Stream()
        if all(planted_bug_is_seen(s, o, cycles_per_ms) for o in (torch.cuda.default_stream(), other) + tuple(against)):
            if passed_over:
                print(f"stream harness: passed over {len(passed_over)} stream(s) on which a planted ordering bug was not seen")
            return s
        passed_over.append(s)
    raise AssertionError("stream harness: a planted ordering bug was not seen on any of eight new streams: the harness is blind here")
