#!/usr/bin/env python3
"""What following points given on a stored frame costs (DenseTrackStore.locate / tracks_from; csrc/trackstore.hip).

Two sizes: 512 x 512 with the 30-pixel grid (324 points) on the tracker's own results (stand-in weights, synthetic video), and
1080 x 1920 with 2304 points on seeded smooth fields (no tracking there).  The query points are the grid's images on the frame
they are given on, so each has a preimage.  For each size, with all points on one frame and with the same points spread over 50
frames:
  * ``mftx_trackstore_locate`` alone -- the key memset, the search kernel and the resolve kernel, tables already on the device --
    timed with events in batches, microseconds per call;
  * ``store.locate`` (the same plus the grouping on the host and the upload of its tables), events in batches;
  * ``store.tracks_from`` over all frames end to end: host clock, one download, synchronised.
For scale only, at 512 x 512: the alternative without ``locate``, a second tracker pass with frame Q as the template (forward from
Q to the end and backward from Q to the start).
The per-kernel times come from a kernel trace of ``--kernels-only`` (a run of its own under the profiler, which slows the
host); ``--kernel-trace <its kernel_trace.csv>`` folds them into the JSON file.  Writes profiles/track_locate.json.

    python tools/bench_track_locate.py [--frames 60] [--out profiles/track_locate.json]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o locate -- python tools/bench_track_locate.py --kernels-only
    python tools/bench_track_locate.py --kernel-trace <dir>/.../locate_kernel_trace.csv [--out profiles/track_locate.json]
"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from mft_amd import _lib, ops, vis  # noqa: E402
from mft_amd import video as vio  # noqa: E402
from mft_amd.config import load_config  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402
from mft_amd.trackstore import DenseTrackStore  # noqa: E402

DEV = "cuda"
SPREAD = 50
KERNELS = ("ts_locate_search_kernel", "ts_locate_resolve_kernel")


def timed(fn, reps):
    """[(host seconds incl. the final synchronise, device milliseconds between events)] of `reps` calls"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append((time.perf_counter() - t0, a.elapsed_time(b)))
    return out


def smooth_results(H, W, n, seed=0):
    """n seeded smooth results on the device: flows of a few pixels whose gradient stays far below 1 (no folds)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for _ in range(n):
        up = lambda c, amp: torch.nn.functional.interpolate(torch.randn(1, c, 9, 16, generator=g) * amp, size=(H, W), mode="bilinear",  # noqa: E731
                                                            align_corners=True)[0].to(DEV).contiguous()
        out.append((up(2, 12.0), up(1, 0.3).abs().clamp(0, 1).contiguous(), (up(1, 0.7).abs() + 0.05).contiguous()))
    return out


def cases(store, H, W, q_frame):
    """{"one_frame" | "spread_50_frames": (xy device [N, 2], frame ids)}: the grid's images on the frames they are given on"""
    grid = vis.get_queries((H, W), 30).to(DEV).contiguous()
    N = int(grid.shape[0])
    images = store.query(grid)                                          # [N, T, 4], append order = frame order here
    spread = [(q_frame + k) % SPREAD for k in range(N)]
    rows = torch.arange(N, device=DEV)
    return {"one_frame": (images[:, q_frame, 0:2].contiguous(), [q_frame] * N),
            "spread_50_frames": (images[rows, torch.tensor(spread, device=DEV), 0:2].contiguous(), spread)}


def locate_legs(store, H, W, xy, ids, batch, reps):
    lib = _lib.load()
    N = int(xy.shape[0])
    slots = [store.slot_of(f) for f in ids]
    buf, G, off = ops.locate_tables(slots, [c.data_ptr() for c in store._chunks], [l.data_ptr() for l in store._lohi],
                                    store.frames_per_chunk, H * W * 8)
    tables = torch.from_numpy(buf).to(DEV)
    base = tables.data_ptr()
    keys = torch.empty(N, dtype=torch.int64, device=DEV)
    table, cell = torch.empty((N, 4), device=DEV), torch.empty((N,), dtype=torch.int32, device=DEV)

    def c_calls():
        for _ in range(batch):
            _lib.check(lib.mftx_trackstore_locate(base + off[0], base + off[1], base + off[2], G, base + off[3], base + off[4], H, W, N,
                                                  xy.data_ptr(), 0.5, keys.data_ptr(), table.data_ptr(), cell.data_ptr(), ops._stream()),
                       "mftx_trackstore_locate")

    def store_calls():
        for _ in range(batch):
            store.locate(xy, ids, out=(table, cell))

    def end_to_end():
        return store.tracks_from(xy, ids)

    res = {"points": N, "frame_groups": G, "cell_tiles": -(-(W - 1) // 32) * -(-(H - 1) // 8)}
    for name, fn in (("c_call_memset_search_resolve", c_calls), ("store_locate", store_calls)):
        fn()
        t = timed(fn, reps)
        res[name + "_us"] = float(np.median([d for _, d in t]) * 1e3 / batch)
        res[name + "_us_min_max"] = [float(min(d for _, d in t) * 1e3 / batch), float(max(d for _, d in t) * 1e3 / batch)]
        res[name + "_host_us"] = float(np.median([h for h, _ in t]) * 1e6 / batch)
    end_to_end()
    t = timed(end_to_end, reps)
    res["tracks_from_all_frames_ms"] = float(np.median([h for h, _ in t]) * 1e3)
    res["tracks_from_frames"] = len(store)
    found = int((cell >= 0).sum())
    res["found"] = found
    back = store.query(table[:, 0:2])                                     # located points sent forward again, on their own frames
    cols = torch.tensor([store.slot_of(f) for f in ids], device=DEV)
    err = (back[torch.arange(N, device=DEV), cols, 0:2] - xy).abs()
    res["max_abs_round_trip_px"] = float(err[cell >= 0].max()) if found else None
    return res


def upload_streams(tracker):
    up = [torch.cuda.current_stream()]
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    return up


def tracker_pass(tracker, frames, start=0, direction=+1):
    seq = frames[start:] if direction > 0 else frames[start::-1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, dev_frame in enumerate(vio.FrameRing(seq, streams=upload_streams(tracker))):
        if i == 0:
            tracker.init(dev_frame, start_frame_i=start, time_direction=direction)
        else:
            tracker.track(dev_frame)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def build_512(n):
    config = load_config(REPO / "configs" / "MFT_cfg.py")
    config.flow_config.model = None
    config.flow_config.synthetic_weights_seed = 0
    config.keep_result_on_device = True
    config.track_store = True
    tracker = config.tracker_class(config)
    src = SyntheticVideo(512, 512, n_frames=n, seed=0)
    frames = [src[i] for i in range(n)]
    tracker_pass(tracker, frames[:20])                                   # warm-up: graphs captured, buffers pinned
    tracker_pass(tracker, frames)
    return tracker, frames, tracker.track_store


def build_1080p(n):
    H, W = 1080, 1920
    fields = smooth_results(H, W, 8)
    store = DenseTrackStore(H, W, device=DEV)
    for k in range(n):
        store.append(fields[k % 8], k)
    return store


TRACE_CASES = ("512x512 one_frame", "512x512 spread_50_frames", "1080x1920 one_frame", "1080x1920 spread_50_frames")
TRACE_CALLS = 20


def fold_kernel_trace(path, out):
    """rocprofv3's kernel_trace.csv of a --kernels-only run -> "kernel_trace" of the JSON file: that run makes TRACE_CALLS calls
    per case, the cases in the order of TRACE_CASES, so the dispatches of each kernel fall into four runs of TRACE_CALLS."""
    report = json.loads(out.read_text()) if out.exists() else {}
    spans = {k: [] for k in KERNELS}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    spans[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    trace = {}
    for k, sp in spans.items():
        sp.sort()
        assert len(sp) == TRACE_CALLS * len(TRACE_CASES), (k, len(sp))
        for c, case in enumerate(TRACE_CASES):
            us = [(e - s) / 1e3 for s, e in sp[c * TRACE_CALLS:(c + 1) * TRACE_CALLS]]
            trace.setdefault(case, {})[k + "_us"] = {"median": float(np.median(us)), "min": float(min(us)), "max": float(max(us))}
    report["kernel_trace"] = {"what": "rocprofv3 --kernel-trace of --kernels-only (smooth fields at both sizes, %d calls per case), a run of its own" % TRACE_CALLS,
                              "cases": trace}
    out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernels-only", action="store_true", help="smooth fields at both sizes, 20 locate calls per case, nothing written: for a kernel trace")
    ap.add_argument("--kernel-trace", type=Path, default=None, help="fold the kernel_trace.csv of a --kernels-only run into the JSON file (needs no GPU)")
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_locate.json")
    args = ap.parse_args()
    if args.kernel_trace is not None:
        return fold_kernel_trace(args.kernel_trace, args.out)
    assert torch.cuda.is_available(), "bench_track_locate.py measures on the GPU"
    assert args.frames >= SPREAD, f"the spread case wants {SPREAD} stored frames"
    torch.cuda.set_device(0)
    n, q_frame = args.frames, args.frames // 2
    if args.kernels_only:
        for H, W in ((512, 512), (1080, 1920)):
            store = DenseTrackStore(H, W, device=DEV)
            for k, r in enumerate(smooth_results(H, W, 8) * 7):
                if k < SPREAD:
                    store.append(r, k)
            for xy, ids in cases(store, H, W, SPREAD // 2).values():
                for _ in range(TRACE_CALLS):
                    store.locate(xy, ids)
            torch.cuda.synchronize()
        return
    report = {"what": "DenseTrackStore.locate / tracks_from: points given on stored frames; events in batches of %d, median of %d" % (args.batch, args.reps),
              "device": torch.cuda.get_device_name(0), "stored_frames": n, "query_frame": q_frame}
    tracker, frames, store = build_512(n)
    report["512x512_tracker_results"] = {name: locate_legs(store, 512, 512, xy, ids, args.batch, args.reps)
                                         for name, (xy, ids) in cases(store, 512, 512, q_frame).items()}
    tracker.C.track_store = False
    fwd = [tracker_pass(tracker, frames, q_frame, +1) for _ in range(3)]
    bwd = [tracker_pass(tracker, frames, q_frame, -1) for _ in range(3)]
    report["512x512_second_tracker_pass_from_frame_q"] = {"forward_frames": n - q_frame, "backward_frames": q_frame + 1,
                                                         "forward_s": float(np.median(fwd)), "backward_s": float(np.median(bwd)),
                                                         "total_ms": float((np.median(fwd) + np.median(bwd)) * 1e3)}
    del tracker, store
    big = build_1080p(n)
    report["1080x1920_smooth_fields"] = {name: locate_legs(big, 1080, 1920, xy, ids, args.batch, args.reps)
                                         for name, (xy, ids) in cases(big, 1080, 1920, q_frame).items()}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
