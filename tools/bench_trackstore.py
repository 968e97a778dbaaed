#!/usr/bin/env python3
"""What the dense track store (mft_amd/trackstore.py, csrc/trackstore.hip) costs and what it buys.

Seeded stand-in weights, the seeded synthetic video, the shipped configuration (12 iterations, seven deltas).  In one process,
every comparison alternating a, b, a, b, a, b:
  (a) the tracking loop at 512 x 512 with ``config.track_store`` off and on (frames/s; the store appends every frame's result);
  (b) the read-out of a 30-pixel query grid over ALL frames after the pass: ``store.query`` -- one call on the 8 B/px store --
      against what there was before: the fp32 results kept on the device at 16 B/px and one ``ops.sample_points`` launch per frame
      into the same [N, T, 4] table.  At 512 x 512 on the tracker's own results; at 1080 x 1920 on seeded smooth fields (no
      tracking there: only the store and the read-outs are measured);
  (c) ``append`` and ``query`` alone, timed with events in batches, with their algorithmic bytes (append: 16 B/px read twice +
      8 B/px written; query: 32 B of taps + 16 B written per point and frame) against the 6.29 TB/s HBM figure of this project;
  (d) the bytes held per frame, both ways.
Writes one JSON file (default profiles/trackstore.json).

    python tools/bench_trackstore.py [--frames 200] [--rounds 3] [--out profiles/trackstore.json]
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

from mft_amd import ops, vis  # noqa: E402
from mft_amd import video as vio  # noqa: E402
from mft_amd.config import load_config  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402
from mft_amd.trackstore import DenseTrackStore  # noqa: E402

HBM_TBS = 6.29
DEV = "cuda"


def upload_streams(tracker):
    up = [torch.cuda.current_stream()]
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    return up


def leg_tracker(tracker, frames, store, keep=False):
    """The tracking loop; results stay on the device.  ``keep``: collect every frame's fp32 result (what a caller without the
    store has to hold for a read-out after the pass)."""
    tracker.C.track_store = bool(store)
    kept = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=upload_streams(tracker))):
        meta = tracker.init(dev_frame) if i == 0 else tracker.track(dev_frame)
        if keep:
            kept.append(tuple(p.to(DEV) for p in meta.result.planes()))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    return {"seconds": seconds, "fps": len(frames) / seconds}, kept


def smooth_results(H, W, n, seed=0):
    """n seeded smooth results on the device (for the sizes that are not tracked here)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for _ in range(n):
        up = lambda c, amp: torch.nn.functional.interpolate(torch.randn(1, c, 9, 16, generator=g) * amp, size=(H, W), mode="bilinear",  # noqa: E731
                                                            align_corners=True)[0].to(DEV).contiguous()
        out.append((up(2, 12.0), up(1, 0.3).abs().clamp(0, 1).contiguous(), (up(1, 0.7).abs() + 0.05).contiguous()))
    return out


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


def query_legs(store, results, H, W, spacing, rounds):
    """(b): one store.query against one sample_points launch per frame, alternating; both fill an [N, T, 4] table"""
    xy = vis.get_queries((H, W), spacing).to(DEV).contiguous()
    N, T = int(xy.shape[0]), len(store)
    tmpl = torch.zeros(N, dtype=torch.int32, device=DEV)
    t_store = torch.zeros((N, T, 4), device=DEV)
    t_fp32 = torch.zeros((N, T, 4), device=DEV)

    def a():
        store.query(xy, out=t_store)

    def b():
        for j, r in enumerate(results):
            ops.sample_points([r], tmpl, xy, t_fp32, j)

    a(); b()                                                            # warm-up
    legs = []
    for _ in range(rounds):
        ta, tb = timed(a, 5), timed(b, 5)
        legs.append({"store_query_ms": float(np.median([h for h, _ in ta]) * 1e3), "store_query_device_ms": float(np.median([d for _, d in ta])),
                     "fp32_per_frame_ms": float(np.median([h for h, _ in tb]) * 1e3), "fp32_per_frame_device_ms": float(np.median([d for _, d in tb]))})
    diff = (t_store - t_fp32).abs()
    return {"points": N, "frames": T, "rounds": legs,
            "speedup_host_clock": float(np.median([r["fp32_per_frame_ms"] / r["store_query_ms"] for r in legs])),
            "max_abs_difference_xy_px": float(diff[..., 0:2].max()), "max_abs_difference_occlusion": float(diff[..., 2].max()),
            "max_abs_difference_sigma": float(diff[..., 3].max())}, xy


def kernel_timings(store, results, xy, H, W, batch=20, reps=15):
    """(c): event timings of batches of `batch` launches, microseconds per launch (median over `reps` batches)"""
    scratch = DenseTrackStore(H, W, device=DEV, frames_per_chunk=batch)
    for k in range(batch):
        scratch.append(results[k % len(results)], k)
    N, T = int(xy.shape[0]), len(store)
    table = torch.zeros((N, T, 4), device=DEV)
    slots = torch.arange(T, dtype=torch.int32, device=DEV)

    def appends():
        for k in range(batch):
            ops.trackstore_append(results[k % len(results)], scratch.packed(k), scratch.lohi(k))

    def queries():
        for _ in range(batch):
            ops.trackstore_query(store._chunks, store._lohi, slots, xy, table, 0)

    def unpacks(out=ops.trackstore_unpack(scratch.packed(0), scratch.lohi(0))):
        for k in range(batch):
            ops.trackstore_unpack(scratch.packed(k), scratch.lohi(k), out=out)

    res = {}
    for name, fn, nbytes in (("append", appends, 40.0 * H * W), ("query", queries, 48.0 * N * T), ("unpack", unpacks, 24.0 * H * W)):
        fn()
        us = float(np.median([d for _, d in timed(fn, reps)]) * 1e3 / batch)
        res[name] = {"us_per_call": us, "algorithmic_bytes": nbytes, "achieved_tb_per_s": nbytes / (us * 1e-6) / 1e12,
                     "fraction_of_hbm_6.29_tb_per_s": nbytes / (us * 1e-6) / 1e12 / HBM_TBS}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid_spacing", type=int, default=30)
    ap.add_argument("--no-1080p", action="store_true")
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "trackstore.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trackstore.py measures on the GPU"
    torch.cuda.set_device(0)
    config = load_config(REPO / "configs" / "MFT_cfg.py")
    config.flow_config.model = None
    config.flow_config.synthetic_weights_seed = 0
    config.keep_result_on_device = True
    tracker = config.tracker_class(config)
    H = W = 512
    n = args.frames
    src = SyntheticVideo(H, W, n_frames=n, seed=0)
    frames = [src[i] for i in range(n)]

    leg_tracker(tracker, frames[:40], store=False)                       # warm-up: graphs captured, buffers pinned
    leg_tracker(tracker, frames[:40], store=True)
    rounds = []
    for _ in range(args.rounds):
        off, _ = leg_tracker(tracker, frames, store=False)
        on, _ = leg_tracker(tracker, frames, store=True)
        rounds.append({"store_off": off, "store_on": on})
    store = tracker.track_store                                          # the last pass' store: n frames
    assert len(store) == n
    _, kept = leg_tracker(tracker, frames, store=False, keep=True)
    offs, ons = [r["store_off"]["fps"] for r in rounds], [r["store_on"]["fps"] for r in rounds]
    report = {"what": "dense track store: tracker with / without it, read-out after the pass, kernels alone; stand-in weights, synthetic video",
              "device": torch.cuda.get_device_name(0), "frames": n,
              "tracker_512": {"rounds": rounds, "fps_store_off_median": float(np.median(offs)), "fps_store_on_median": float(np.median(ons)),
                              "fps_store_off_spread": float(max(offs) - min(offs)), "fps_store_on_spread": float(max(ons) - min(ons)),
                              "store_on_over_off": float(np.median(ons) / np.median(offs))}}
    q512, xy = query_legs(store, kept, H, W, args.grid_spacing, args.rounds)
    report["query_512"] = q512
    report["kernels_512"] = kernel_timings(store, kept, xy, H, W)
    report["bytes_per_frame_512"] = {"store": store.nbytes / (len(store._chunks) * store.frames_per_chunk), "fp32_results": 16 * H * W,
                                     "store_total": store.nbytes, "fp32_total": 16 * H * W * n}
    del kept, store
    tracker.C.track_store = False
    if not args.no_1080p:
        H2, W2 = 1080, 1920
        fields = smooth_results(H2, W2, 8)
        big = DenseTrackStore(H2, W2, device=DEV)
        results = [fields[k % 8] for k in range(n)]                      # the fp32 side reads n distinct addresses only 8 times over:
        results = [tuple(p.clone() for p in r) for r in results]         # ... so every frame gets planes of its own (n x 33 MB)
        for k, r in enumerate(results):
            big.append(r, k)
        q1080, xy2 = query_legs(big, results, H2, W2, args.grid_spacing, args.rounds)
        report["query_1080p"] = q1080
        report["kernels_1080p"] = kernel_timings(big, results, xy2, H2, W2)
        report["bytes_per_frame_1080p"] = {"store": big.nbytes / (len(big._chunks) * big.frames_per_chunk), "fp32_results": 16 * H2 * W2,
                                           "store_total": big.nbytes, "fp32_total": 16 * H2 * W2 * n}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
