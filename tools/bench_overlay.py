#!/usr/bin/env python3
"""What the demo's overlay stage costs, on the host (demo.py as it was) and on the device (``--gpu-overlays``).

512 x 512, seeded stand-in weights, the seeded synthetic video, a seeded RGBA edit over about a third of the frame.  In one
process, alternating a, b, a, b, a, b:
  (a) demo.py's default path: the tracking loop with every dense result downloaded and kept, then ``vis.draw_dots`` +
      ``vis.draw_edit`` per frame on the host;
  (b) demo.py --gpu-overlays: the same loop with ``vis.DeviceOverlay`` rendering inside it, frames downloaded as uint8;
then the tracker alone, and the splat / composite / dots kernels timed one by one with events.  Neither leg writes PNGs (the
encoder is the same host code in both).  Writes one JSON file (default profiles/overlay_device.json).

    python tools/bench_overlay.py [--frames 24] [--rounds 3] [--out profiles/overlay_device.json]
"""
import argparse
import ctypes as C
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
from mft_amd.point_tracking import convert_to_point_tracking  # noqa: E402
from mft_amd.results import FlowOUTrackingResult  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402

H = W = 512


def make_edit(seed=0):
    """B, G, R, A uint8: a random-coloured 300 x 292 patch (a third of the frame), alpha 64..255 with a tenth of it cut out."""
    r = np.random.default_rng(seed)
    edit = np.zeros((H, W, 4), np.uint8)
    edit[100:400, 110:402, :3] = r.integers(0, 256, size=(300, 292, 3), dtype=np.uint8)
    alpha = r.integers(64, 256, size=(300, 292), dtype=np.uint8)
    alpha[r.random((300, 292)) < 0.1] = 0
    edit[100:400, 110:402, 3] = alpha
    return edit


def upload_streams(tracker):
    up = [torch.cuda.current_stream()]
    if getattr(tracker.flower, "_enc_stream", None) is not None:
        up.append(tracker.flower._enc_stream)
    return up


def leg_host(tracker, frames, edit, spacing):
    """demo.py's default path, minus the PNG encoder"""
    t0 = time.perf_counter()
    results, host_results, queries = [], [], None
    drain = vio.ResultDrain()
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=upload_streams(tracker))):
        if i == 0:
            meta = tracker.init(dev_frame)
            meta.result = meta.result.cuda()
            queries = vis.get_queries(frames[0].shape[:2], spacing).cuda()
        else:
            meta = tracker.track(dev_frame)
        coords, occlusions = convert_to_point_tracking(meta.result, queries)
        drain.submit(meta.result)
        host_results.append(FlowOUTrackingResult(*drain.collect(copy=True), validate=False))
        results.append((coords, occlusions))
    t1 = time.perf_counter()
    out = []
    for i, frame in enumerate(frames):
        coords, occlusions = results[i]
        out.append((vis.draw_dots(frame, coords, occlusions), vis.draw_edit(frame, host_results[i], edit)))
    t2 = time.perf_counter()
    return {"seconds": t2 - t0, "tracking_seconds": t1 - t0, "overlay_seconds": t2 - t1}, out


def leg_device(tracker, frames, edit, spacing):
    """demo.py --gpu-overlays, minus the PNG encoder"""
    t0 = time.perf_counter()
    out, overlay = [], None
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=upload_streams(tracker))):
        if i == 0:
            meta = tracker.init(dev_frame)
            meta.result = meta.result.cuda()
            overlay = vis.DeviceOverlay(edit, vis.get_queries(frames[0].shape[:2], spacing), H, W)
        else:
            meta = tracker.track(dev_frame)
        overlay.render(dev_frame, meta.result)
        out += overlay.download()
    out += overlay.download(wait=True)
    seconds = time.perf_counter() - t0
    return {"seconds": seconds}, out, meta.result.clone()


def leg_tracker(tracker, frames):
    t0 = time.perf_counter()
    for i, dev_frame in enumerate(vio.FrameRing(frames, streams=upload_streams(tracker))):
        meta = tracker.init(dev_frame) if i == 0 else tracker.track(dev_frame)
    torch.cuda.synchronize()
    del meta
    return {"seconds": time.perf_counter() - t0}


def count_adds(result, edit):
    """The 64-bit atomic adds the edit splat issues for this result (host restatement of the kernel's drop rules)."""
    flow = result.flow.cpu().numpy()
    keep = (result.occlusion[0].cpu().numpy() < 0.5) & (edit[..., 3] > 0)
    gy, gx = np.mgrid[0:H, 0:W]
    x, y = gx.astype(np.float32) + flow[0], gy.astype(np.float32) + flow[1]
    keep &= np.isfinite(x) & np.isfinite(y)
    x, y = x[keep], y[keep]
    x0, y0 = np.clip(np.floor(x), -1e6, 1e6).astype(np.int64), np.clip(np.floor(y), -1e6, 1e6).astype(np.int64)
    xc, yc = np.clip(x, 0, W - 1).astype(np.float32), np.clip(y, 0, H - 1).astype(np.float32)
    wx0, wx1 = np.clip(x0 + 1, 0, W - 1).astype(np.float32) - xc, xc - np.clip(x0, 0, W - 1).astype(np.float32)
    wy0, wy1 = np.clip(y0 + 1, 0, H - 1).astype(np.float32) - yc, yc - np.clip(y0, 0, H - 1).astype(np.float32)
    S = ops.splat_plan(H, W, 16, False).S
    live = sum(int((np.rint((w.astype(np.float64)) * 2.0 ** S) != 0).sum()) for w in (wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1))
    nonzero_values = (edit[..., :3][keep] != 0).mean() * 3 + 2          # b a, g a, r a (zero products are skipped), a, cnt
    return int(keep.sum()), int(round(live * nonzero_values))


def time_kernels(result, edit, frame, queries, reps=50):
    """Event timings, microseconds per launch (median of `reps`), each kernel alone on an idle stream."""
    lib = _lib.load()
    dev = result.flow.device
    flow, occl = result.flow.contiguous(), result.occlusion.contiguous()
    edit_d, frame_d = torch.from_numpy(edit).to(dev), torch.from_numpy(np.ascontiguousarray(frame)).to(dev)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    acc = ops.splat_accumulator(4, H, W, dev)
    S = ops.splat_plan(H, W, 16, False).S
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    div = ops.edit_alpha_divisor(edit)
    table = torch.zeros(queries.shape[0], 4, device=dev)
    ops.sample_points([result.planes()], torch.zeros(queries.shape[0], dtype=torch.int32, device=dev), queries.to(dev).contiguous(), table, 0)

    def splat():
        _lib.check(lib.mftx_overlay_edit(flow.data_ptr(), occl.data_ptr(), edit_d.data_ptr(), None, H, W, S, div, acc.data_ptr(), None, st), "splat")

    def composite():
        _lib.check(lib.mftx_overlay_edit(None, None, None, frame_d.data_ptr(), H, W, S, div, acc.data_ptr(), out.data_ptr(), st), "composite")

    def dots():
        ops.overlay_dots(frame_d, table, out=out)

    def dots_in_place():
        ops.overlay_dots(out, table, out=out)

    def median_us(fn, before=None):
        ts = []
        for _ in range(reps):
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    for _ in range(3):
        splat(); composite(); dots()
    t = {"edit_splat_us": median_us(splat, before=composite),          # the composite leaves the accumulator zeroed
         "edit_composite_us": median_us(composite, before=splat),
         "dots_with_frame_copy_us": median_us(dots),
         "dots_in_place_us": median_us(dots_in_place)}
    composite()
    torch.cuda.synchronize()
    kept, adds = count_adds(result, edit)
    t.update(kept_source_pixels=kept, atomic_adds=adds, atomic_bytes=8 * adds,
             atomic_gb_per_s=round(8 * adds / (t["edit_splat_us"] * 1e-6) / 1e9, 1))
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid_spacing", type=int, default=30)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "overlay_device.json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    config = load_config(REPO / "configs" / "MFT_cfg.py")
    config.flow_config.model = None
    config.flow_config.synthetic_weights_seed = 0
    config.keep_result_on_device = True
    tracker = config.tracker_class(config)
    src = SyntheticVideo(H, W, n_frames=args.frames, seed=0)
    frames = [src[i] for i in range(args.frames)]
    edit = make_edit()
    n = args.frames

    leg_tracker(tracker, frames[:6])                                  # warm-up: graphs captured, buffers pinned
    leg_device(tracker, frames[:6], edit, args.grid_spacing)
    rounds, last = [], None
    for _ in range(args.rounds):
        a, host_out = leg_host(tracker, frames, edit, args.grid_spacing)
        b, dev_out, last = leg_device(tracker, frames, edit, args.grid_spacing)
        worst = max(int(np.abs(h[1].astype(np.int64) - d[1].astype(np.int64)).max()) for h, d in zip(host_out, dev_out))
        differ = float(np.mean([(h[1] != d[1]).mean() for h, d in zip(host_out, dev_out)]))
        beyond = int(sum((np.abs(h[1].astype(np.int64) - d[1].astype(np.int64)) > 1).sum() for h, d in zip(host_out, dev_out)))
        same_dots = bool(np.array_equal(host_out[0][0], dev_out[0][0]))       # frame 0: the dots sit at the queries in both
        rounds.append({"host_overlays": a, "device_overlays": b, "host_fps": n / a["seconds"], "device_fps": n / b["seconds"],
                       "edit_frames_max_level_difference": worst, "edit_frames_fraction_of_values_differing": differ,
                       "edit_frames_values_more_than_one_level_apart": beyond, "first_point_frame_identical": same_dots})
        del host_out, dev_out
    alone = [leg_tracker(tracker, frames) for _ in range(args.rounds)]
    tracker_fps = n / min(t["seconds"] for t in alone)
    kernels = time_kernels(last, edit, frames[-1], vis.get_queries((H, W), args.grid_spacing))
    best_b = max(r["device_fps"] for r in rounds)
    report = {"what": "demo overlay stage at 512 x 512, stand-in weights, synthetic video; no PNG encoding in either leg",
              "device": torch.cuda.get_device_name(0), "frames": n, "rounds": rounds,
              "device_beats_host_in_every_round": all(r["device_fps"] > r["host_fps"] for r in rounds),
              "tracker_alone_fps": tracker_fps, "tracker_alone_seconds": [t["seconds"] for t in alone],
              "device_overlays_fraction_of_tracker_alone": best_b / tracker_fps,
              "kernels": kernels}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
