"""Stream ordering of the stateless entry points of mft_amd/ops.py (tests/stream_catalog.py: one entry each).

Per entry: the call is made on a fresh side stream that is kept busy by a bounded spin, with its inputs rewritten on that stream
behind the spin.  A launcher that ignored its ``stream`` argument, a wrapper that forgot to pass it, or a helper copy issued on
another stream would run while the spin is still going and read the input set the buffers held before -- a different, valid input
set, so a different answer.  The expected answer is the same call on the new input set, synchronous, on the default stream, on
tensors of its own, computed AFTER the stalled run: no arithmetic is compared with anything but itself.

The completeness test at the end needs no GPU: every function of ops.py that names ``_stream()`` is in the catalog, in the handle
tests (tests/test_gpu_streams_handles.py), or exempt with a reason.
"""
import ast
import itertools
from pathlib import Path

import pytest
import torch

import stream_catalog as cat
import stream_harness as sh

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda"
_SEEDS = itertools.count(40_000)          # every test takes input seeds nothing else in the process has used


@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def rewrite(dst, src):
    """dst <- src in place on the current stream (16-bit samples through their int16 views)."""
    for k in dst:
        assert dst[k].is_contiguous() and src[k].is_contiguous() and dst[k].shape == src[k].shape, k
        sh.as_bits(dst[k]).copy_(sh.as_bits(src[k]), non_blocking=True)


def snapshot(outs):
    """Copies of the outputs enqueued on the current stream, behind the call (pinned host outputs: an upload)."""
    return [o.clone() if o.is_cuda else o.to(DEV, non_blocking=True) for o in outs]


def differs(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a, b))


def run_behind_stall(ops, e, cycles_per_ms, variants=(0,)):
    """Steps 1-4 for one entry -> nothing; asserts.  variants (0, 1): two calls back to back behind ONE stall."""
    fx = e.fixed(ops)
    stale, fresh = to_dev(e.inputs(ops, next(_SEEDS))), to_dev(e.inputs(ops, next(_SEEDS)))
    side = sh.visible_stream(cycles_per_ms)                    # (a stream on which work that lands on the null stream is not serialised)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        inp = {k: v.clone() for k, v in stale.items()}
        # the unstalled warm-up, on the old input set: its host time sizes the stall, and its answer is what a call that ran too
        # early would give again
        old, host = sh.timed(lambda: [e.call(ops, fx, inp, v) for v in variants])
        side.synchronize()
        old = [sh.host_copies(o) for o in old]
        rewrite(inp, stale)                                    # (entries that write into an input)
        side.synchronize()
        ms = sh.stall_ms(host)
        stall_end = sh.stall(side, ms, cycles_per_ms)
        rewrite(inp, fresh)
        outs = [e.call(ops, fx, inp, v) for v in variants]
        behind = sh.enqueued_behind(stall_end)                 # immediately after the product call returned
        snaps = [snapshot(o) for o in outs]
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()                                         # the event only: no device-wide synchronisation before reading
    got = [sh.host_copies(o) for o in outs]
    got_snap = [sh.host_copies(s) for s in snaps]
    torch.cuda.synchronize()
    print(f"{e.name}: warm-up took {1e3 * host:.2f} ms on the host, stalled for {ms:.0f} ms, enqueued behind the stall: {behind}")
    if e.host_wait is None:
        assert behind, (f"{e.name}: the stall of {ms:.0f} ms had ended when the call returned: nothing is proven; the call waited for the "
                        "host, or the host was slower than four times its warm-up")
    # the reference: the same calls where no race is possible, on tensors of their own
    ref_in = {k: v.clone() for k, v in fresh.items()}
    torch.cuda.synchronize()
    want = []
    for v in variants:
        want.append(sh.host_copies(e.call(ops, fx, ref_in, v)))
        torch.cuda.synchronize()
    assert any(differs(w, o) for w, o in zip(want, old)), f"{e.name}: the two input sets give the same answer: the test could not see a stale read"
    for v, w, g, s in zip(variants, want, got, got_snap):
        for i, (wi, gi_, si) in enumerate(zip(w, g, s)):
            assert wi.shape == gi_.shape and wi.dtype == gi_.dtype, (e.name, v, i)
            assert torch.equal(gi_, wi), (f"{e.name} call {v} output {i}: {int((gi_ != wi).sum())} of {wi.numel()} elements differ from the "
                                         "race-free run: the call ran elsewhere or too early")
            assert torch.equal(si, wi), (f"{e.name} call {v} output {i}: the same-stream copy differs in {int((si != wi).sum())} elements: "
                                         "the result was not ordered in front of the stream's next work")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("e", cat.ENTRIES, ids=lambda e: e.name)
def test_entry_point_runs_on_its_stream(ops, cycles_per_ms, e):
    run_behind_stall(ops, e, cycles_per_ms)


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("e", [e for e in cat.ENTRIES if e.tables], ids=lambda e: e.name)
def test_table_uploads_back_to_back(ops, cycles_per_ms, e):
    """Two calls with different host tables behind ONE stall: the second call's pinned temporary must not replace the first's before
    the first has been copied to the device (ops._upload_tables drops its pinned buffer right after an asynchronous copy)."""
    run_behind_stall(ops, e, cycles_per_ms, variants=(0, 1))


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_harness_sees_a_planted_ordering_bug(ops, cycles_per_ms):
    """The negative control of this file: ``ops.copy_bytes`` called under another stream than the current one -- the null stream, where
    a launcher that ignored its stream argument would land, and a side stream -- is reported.  If not, the tests above prove nothing."""
    side = sh.visible_stream(cycles_per_ms)
    for other in (torch.cuda.default_stream(), torch.cuda.Stream()):
        assert sh.planted_bug_is_seen(side, other, cycles_per_ms, copy=ops.copy_bytes, n=125 * 187 + 3), \
            "the harness is blind in this process: a copy made on another stream, in front of the rewrite of its source, was not seen"
    torch.cuda.synchronize()


# ---- completeness: no GPU ---------------------------------------------------------------------------------------------------------
def _names_stream(fn):
    return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_stream" for n in ast.walk(fn))


def streamed_entry_points():
    """Every module-level function of mft_amd/ops.py, and every method of EncoderEngine / RaftEngine (as 'Class.method'), whose body
    calls ``_stream()``."""
    tree = ast.parse((REPO / "mft_amd" / "ops.py").read_text())
    found = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name != "_stream" and _names_stream(node):
            found.append(node.name)
        if isinstance(node, ast.ClassDef) and node.name in ("EncoderEngine", "RaftEngine"):
            found += [f"{node.name}.{m.name}" for m in node.body if isinstance(m, ast.FunctionDef) and _names_stream(m)]
    return found


def test_catalog_names_every_streamed_entry_point():
    from mft_amd import ops as ops_mod
    found = streamed_entry_points()
    assert len(found) >= 40 and "copy_bytes" in found and "RaftEngine.refine" in found, found      # the walk itself works
    known = cat.covered() | set(cat.HANDLE_TESTS) | set(cat.EXEMPT)
    missing = [n for n in found if n not in known]
    assert not missing, f"no stream-ordering test for {missing}: add an entry to tests/stream_catalog.py (or a reasoned EXEMPT)"
    for name in cat.covered():
        assert callable(getattr(ops_mod, name)), name
    gone = [n for n in cat.EXEMPT if n not in found]
    assert not gone, f"EXEMPT names {gone}, which no longer hand _stream() to the library"
    assert all(isinstance(r, str) and len(r) > 20 for r in cat.EXEMPT.values())
    handle_tests = {n.name for n in ast.parse((REPO / "tests" / "test_gpu_streams_handles.py").read_text()).body if isinstance(n, ast.FunctionDef)}
    assert set(cat.HANDLE_TESTS.values()) <= handle_tests, set(cat.HANDLE_TESTS.values()) - handle_tests
    # an entry that covers a wrapper covers what the wrapper runs: the public names whose body is another function's
    assert {"trackstore_locate", "trackstore_locate_frames", "split_activations"} <= cat.covered()
    assert len({e.name for e in cat.ENTRIES}) == len(cat.ENTRIES)
