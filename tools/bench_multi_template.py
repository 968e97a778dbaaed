#!/usr/bin/env python3
"""The TAP-Vid 'strided' protocol on one synthetic sequence, two ways, timed against each other in ONE process:

  (a) ``tapvid.run_sequence``: one complete tracker run per start frame and direction, all runs sharing an in-HBM flow cache
      (the sequential path; what tools/run_tapvid_synth.py times);
  (b) ``tapvid.run_sequence_multi``: all start frames of a direction in one lockstep pass (``mft_amd/multi.py``).

Seeded ``SyntheticVideo(512, 512)``, 50 frames, the shipped configuration (12 RAFT iterations, seven deltas), seeded synthetic
weights, queries at every fifth frame (10 start frames, each tracked forward and backward).  A host clock around work that ends
in a device synchronise; one untimed round of each, then a, b, a, b, a, b.  Prints one JSON line.

    python tools/bench_multi_template.py [--frames 50] [--size 512] [--rounds 3] [--out profiles/multi_template_tapvid.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from mft_amd import tapvid  # noqa: E402
from mft_amd.config import load_config  # noqa: E402
from mft_amd.io import FlowCache  # noqa: E402
from mft_amd.multi import MultiTemplateMFT  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402


class CountingCache(FlowCache):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.hits = self.misses = 0

    def read(self, left_id, right_id):
        val = super().read(left_id, right_id)
        if val[0] is None:
            self.misses += 1
        else:
            self.hits += 1
        return val


class CountingMulti(MultiTemplateMFT):
    """Sums the per-pass counters of the tracker over the passes of a protocol run."""
    totals = None

    def point_tracks(self):
        out = super().point_tracks()
        for k, v in self.stats.items():
            self.totals[k] = self.totals.get(k, 0) + v
        self.totals["passes"] = self.totals.get("passes", 0) + 1
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--points", type=int, default=8, help="query points per start frame")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gpu-cache-gb", type=float, default=64.0)
    ap.add_argument("--out", type=Path, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multi_template.py needs a GPU")
    conf = load_config(REPO / "configs" / "MFT_cfg.py")
    conf.flow_config.model = None
    conf.flow_config.synthetic_weights_seed = 0
    conf.flow_config.flow_iters = a.iters
    conf.keep_result_on_device = True
    vid = SyntheticVideo(a.size, a.size, n_frames=a.frames, seed=100)
    video = [np.ascontiguousarray(vid[i]) for i in range(a.frames)]
    rng = np.random.default_rng(0)
    starts = list(range(0, a.frames, a.stride))
    q = np.concatenate([np.stack([np.full(a.points, t), rng.integers(0, a.size, a.points), rng.integers(0, a.size, a.points)], 1)
                        for t in starts]).astype(np.int64)
    tracker_frames = sum((a.frames - s) + (s + 1) for s in starts)
    single = conf.tracker_class(conf)
    multi = CountingMulti(conf)
    cache_stats = {}

    def run_a():
        cache = CountingCache(None, max_GPU_RAM_MB=a.gpu_cache_gb * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tapvid.run_sequence(single, video, q, "strided", flow_cache=cache, device="cuda")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        cache_stats.update(pairs_from_cache=cache.hits, pairs_not_in_cache=cache.misses)
        cache.clear(clear_disk=False)
        return dt, out

    def run_b():
        multi.totals = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tapvid.run_sequence_multi(multi, video, q, "strided", device="cuda")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run_a()
    run_b()                                               # one untimed round of each
    ta, tb = [], []
    for _ in range(a.rounds):
        dt, out_a = run_a()
        ta.append(dt)
        dt, out_b = run_b()
        tb.append(dt)
    ma, mb = statistics.median(ta), statistics.median(tb)
    spread_a = max(ta) - min(ta)
    res = {
        "workload": f"TAP-Vid 'strided' protocol, synthetic {a.size}x{a.size}, {a.frames} frames, {len(starts)} start frames "
                    f"(stride {a.stride}) forward + backward, {a.points} queries each, {a.iters} RAFT iters, {len(conf.deltas)} deltas",
        "device": torch.cuda.get_device_name(0),
        "tracker_frames": tracker_frames,
        "sequential_seconds": ta, "multi_template_seconds": tb,
        "sequential_median_s": ma, "multi_template_median_s": mb,
        "sequential_spread_s": spread_a,
        "speedup": ma / mb,
        "faster_by_more_than_the_spread": bool(ma - mb > spread_a),
        "sequential_frames_per_s": tracker_frames / ma, "multi_template_frames_per_s": tracker_frames / mb,
        "sequential_flow_pairs": cache_stats,
        "multi_template_counts_per_protocol_run": multi.totals,
        "max_track_difference_px_256_raster": float(np.abs(out_a["tracks"] - out_b["tracks"]).max()),
        "max_occlusion_difference": float(np.abs(out_a["occluded"] - out_b["occluded"]).max()),
    }
    line = json.dumps(res)
    print(line)
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")
    if not res["faster_by_more_than_the_spread"]:
        sys.exit("the lockstep pass is NOT faster than the sequential protocol by more than the spread of the sequential runs")


if __name__ == "__main__":
    main()
