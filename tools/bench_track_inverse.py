#!/usr/bin/env python3
"""What inverting stored frames densely costs (DenseTrackStore.inverse / results_from; csrc/trackstore.hip).

``mftx_trackstore_invert`` (a: the key memset, the scatter kernel, the resolve kernel) against the only other way to the same bits
(b): ``mftx_trackstore_locate`` with the H * W pixel centres of every frame as its queries, tables and queries already on the
device.  Both are timed in ONE process, a, b, a, b, a, b, with events around batches of calls (a batch is sized to about 50 ms from
a first call, so the slow side is not run more often than it needs); the medians and their ratio are reported, and the two
results are compared bit for bit.  Two sizes: 512 x 512 on the tracker's own stored results (stand-in weights, synthetic
video) and 1080 x 1920 on seeded smooth fields; one frame and 50 frames per call.  Also: ``store.inverse`` (the call plus its
pinned pointer table), ``store.results_from`` over all stored frames end to end (host clock, synchronised), and what the
scatter kernel met -- the share of cells it walked with a whole wave (more than 16 pixel centres in the cell's range) and the
largest range.  Writes profiles/track_inverse.json.

    python tools/bench_track_inverse.py [--frames 60] [--out profiles/track_inverse.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from mft_amd import _lib, ops  # noqa: E402
from bench_track_locate import build_512, build_1080p  # noqa: E402

DEV = "cuda"
MANY = 50
INLINE = 16                       # csrc/trackstore.hip: TI_INLINE
EPS = 2.0 ** -10
ROUNDS = 3
BATCH_MS = 50.0
SLOW_MS = 1000.0


def device_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def batch_for(fn):
    """calls per timed batch: about BATCH_MS of device time, from a first (warm-up) call and a second, timed one"""
    fn()
    return max(1, min(200, int(BATCH_MS / max(device_ms(fn), 1e-3))))


def interleaved(fa, fb):
    """-> microseconds per call of a and of b: medians over ROUNDS rounds a, b, a, b, ..., events around each batch.  (A side
    whose single call takes longer than SLOW_MS is timed once per round, no warm-up call before.)"""
    na = batch_for(fa)
    first_b = device_ms(fb)
    nb = 1 if first_b > SLOW_MS else batch_for(fb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(device_ms(lambda: [fa() for _ in range(na)]) * 1e3 / na)
        tb.append(device_ms(lambda: [fb() for _ in range(nb)]) * 1e3 / nb)
    return {"invert_us": float(np.median(ta)), "invert_us_min_max": [float(min(ta)), float(max(ta))], "invert_calls_per_batch": na,
            "dense_locate_us": float(np.median(tb)), "dense_locate_us_min_max": [float(min(tb)), float(max(tb))],
            "dense_locate_calls_per_batch": nb, "dense_locate_over_invert": float(np.median(tb) / np.median(ta))}


def pixel_grid(H, W):
    idx = torch.arange(H * W, device=DEV)
    return torch.stack([idx % W, torch.div(idx, W, rounding_mode="floor")], dim=1).to(torch.float32)


def box_stats(store, ids):
    """What the scatter kernel walks on these frames: per cell the pixel centres in the integer range of its widened box."""
    H, W = store.H, store.W
    big = total = largest = walked = 0
    for f in ids:
        r = store.result(f)
        mx = torch.arange(W, device=DEV, dtype=torch.float32)[None, :] + r.flow[0]
        my = torch.arange(H, device=DEV, dtype=torch.float32)[:, None] + r.flow[1]

        def span(m, n):
            c = torch.stack([m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]])
            lo, hi = c.amin(0) - EPS, c.amax(0) + EPS
            return (torch.ceil(hi).clamp(-1, n - 1) - torch.floor(lo).clamp(0, n) + 1).clamp(min=0).to(torch.int64)

        count = span(mx, W) * span(my, H)
        big += int((count > INLINE).sum())
        total += count.numel()
        walked += int(count.sum())
        largest = max(largest, int(count.max()))
    return {"cells": total, "cells_walked_by_a_wave": big, "share_walked_by_a_wave": big / total, "largest_range": largest,
            "centres_tested_per_cell": walked / total}


def legs(store, ids):
    """One set of frames: the two C calls interleaved, the results compared, ``store.inverse``."""
    lib = _lib.load()
    H, W, G = store.H, store.W, len(ids)
    N = G * H * W
    slots = np.asarray([store.slot_of(f) for f in ids], dtype=np.int64)
    fpc = store.frames_per_chunk
    cptr = np.asarray([c.data_ptr() for c in store._chunks], dtype=np.int64)
    lptr = np.asarray([l.data_ptr() for l in store._lohi], dtype=np.int64)
    ptrs = torch.from_numpy(np.concatenate([cptr[slots // fpc] + (slots % fpc) * (H * W * 8), lptr[slots // fpc] + (slots % fpc) * 32])).to(DEV)
    base = ptrs.data_ptr()
    keys = torch.empty(N, dtype=torch.int64, device=DEV)
    table_a, cell_a = torch.empty((G, H, W, 4), device=DEV), torch.empty((G, H, W), dtype=torch.int32, device=DEV)
    table_b, cell_b = torch.empty((N, 4), device=DEV), torch.empty((N,), dtype=torch.int32, device=DEV)
    # dense locate's own inputs: the pixel grid once per frame, the groups in order
    xy = pixel_grid(H, W).repeat(G, 1).contiguous()
    group_start = (torch.arange(G + 1, device=DEV, dtype=torch.int64) * (H * W)).to(torch.int32)
    order = torch.arange(N, device=DEV, dtype=torch.int32)
    group_of = torch.arange(G, device=DEV, dtype=torch.int32).repeat_interleave(H * W).contiguous()

    def invert():
        _lib.check(lib.mftx_trackstore_invert(base, base + 8 * G, G, H, W, 0.5, keys.data_ptr(), table_a.data_ptr(), cell_a.data_ptr(),
                                              ops._stream()), "mftx_trackstore_invert")

    def dense_locate():
        _lib.check(lib.mftx_trackstore_locate(base, base + 8 * G, group_start.data_ptr(), G, order.data_ptr(), group_of.data_ptr(), H, W, N,
                                              xy.data_ptr(), 0.5, keys.data_ptr(), table_b.data_ptr(), cell_b.data_ptr(), ops._stream()),
                   "mftx_trackstore_locate")

    res = {"frames_per_call": G, "pixels": N, "cell_tiles": -(-(W - 1) // 32) * -(-(H - 1) // 8) * G}
    res.update(interleaved(invert, dense_locate))
    same = bool(torch.equal(cell_a.reshape(-1), cell_b) and torch.equal(table_a.reshape(-1, 4).view(torch.int32), table_b.view(torch.int32)))
    res["same_bits"] = same
    res["found_share"] = float((cell_a >= 0).float().mean())
    del xy, order, group_of, table_b, cell_b

    def store_inverse():
        store.inverse(list(ids), out=(table_a, cell_a))

    n = batch_for(store_inverse)
    res["store_inverse_us"] = float(np.median([device_ms(lambda: [store_inverse() for _ in range(n)]) * 1e3 / n for _ in range(ROUNDS)]))
    # the traffic the call cannot avoid: each packed frame once, the keys set, lowered and read, rows and cells written
    res["bytes_moved_at_least"] = int(N * (8 + 8 + 8 + 8 + 16 + 4))
    res["invert_gb_per_s_at_least"] = res["bytes_moved_at_least"] / (res["invert_us"] * 1e-6) / 1e9
    res.update(box_stats(store, ids))
    return res


def results_from_leg(store, src):
    def run():
        out = store.results_from(src)
        torch.cuda.synchronize()
        return out

    run()
    t = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        t.append(time.perf_counter() - t0)
    return {"source_frame": src, "frames": len(store), "results_from_all_frames_ms": float(np.median(t) * 1e3),
            "found_share": float(out[3].float().mean())}


def size_report(store, q_frame):
    return {"one_frame": legs(store, [q_frame]), "many_frames": legs(store, list(range(MANY))),
            "results_from": results_from_leg(store, q_frame)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_inverse.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_inverse.py measures on the GPU"
    assert args.frames >= MANY, f"the many-frames case wants {MANY} stored frames"
    torch.cuda.set_device(0)
    n, q_frame = args.frames, args.frames // 2
    report = {"what": "mftx_trackstore_invert against mftx_trackstore_locate on the pixel grid: a, b, a, b, a, b in one process, events "
                      "around batches of about %g ms, medians of %d; microseconds per call" % (BATCH_MS, ROUNDS),
              "device": torch.cuda.get_device_name(0), "stored_frames": n, "one_frame": q_frame, "many_frames": MANY}
    tracker, frames, store = build_512(n)
    report["512x512_tracker_results"] = size_report(store, q_frame)
    del tracker, frames, store
    torch.cuda.empty_cache()
    report["1080x1920_smooth_fields"] = size_report(build_1080p(n), q_frame)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
