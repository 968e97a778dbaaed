#!/usr/bin/env python3
"""What reading the video along every track costs (``DenseTrackStore.appearance``; csrc/trackstore.hip: ts_appearance_kernel
through ``mftx_trackstore_appearance``).

The fused call against the composition it replaces on the device -- per column ``store.result`` (unpack), ``warp_backward`` and the
torch elementwise mask and sums (``DenseTrackStore._compose_appearance``, the ``device="cpu"`` path's code on device tensors) --
a, b, a, b, a, b in ONE process, events around batches, medians.  The two results are compared as the GPU tests compare them: bit
for bit.

Cases: 512 x 512 x 3, a 200-frame tracker pass (stand-in weights) on the pass's own store and the pass's own video, the template
frame as the reference, over the first 50 frames and over all 200; 1080 x 1920 x 3, 50 frames of seeded smooth fields and seeded
frames; each with and without the per-column stack.  Per case: time per call, the bytes the call cannot avoid -- per pixel and
column the packed word and C image bytes (8 + C), with the stack C + 1 bytes written; per pixel the reference and the results -- with
the rate they imply against 6.29 TB/s, the launch alone (``mftx_trackstore_appearance`` on tables uploaded and results allocated once:
no wrapper, no upload, no allocation), and the peak bytes allocated on both sides.  (The kernel keeps 4 columns in flight; builds with
2 and 8 were measured when that was chosen: profiles/track_appearance_in_flight.json.)

Writes profiles/track_appearance.json.

    python tools/bench_track_appearance.py [--out profiles/track_appearance.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from mft_amd import _lib, ops  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402
from mft_amd.trackstore import DenseTrackStore  # noqa: E402
from bench_track_atlas import config, peak_bytes  # noqa: E402
from bench_track_inverse import batch_for, device_ms  # noqa: E402
from bench_track_locate import smooth_results  # noqa: E402

DEV = "cuda"
ROUNDS = 3
HBM = 6.29e12


def legs(fa, fb):
    """-> (microseconds per call of a, of b, their (min, max)): a, b, a, b, a, b, events around batches of about 50 ms."""
    na, nb = batch_for(fa), batch_for(fb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(device_ms(lambda: [fa() for _ in range(na)]) * 1e3 / na)
        tb.append(device_ms(lambda: [fb() for _ in range(nb)]) * 1e3 / nb)
    return float(np.median(ta)), float(np.median(tb)), [float(min(ta)), float(max(ta))], [float(min(tb)), float(max(tb))]


def same_bits(got, want, stack):
    ok = bool(torch.equal(got.count, want[2])) and all(bool(torch.equal(g.view(torch.int32), w.view(torch.int32)))
                                                       for g, w in ((got.sum, want[0]), (got.sumsq, want[1])))
    if stack:
        ok = ok and bool(torch.equal(got.warped, want[3])) and bool(torch.equal(got.visible, want[4]))
    return ok


def appearance_case(st, frames, images, reference, stack):
    H, W, T, C = st.H, st.W, len(frames), int(images[0].shape[2])
    slots = st._slots(frames)
    fused = lambda: st.appearance(images, frames, reference=reference, stack=stack)  # noqa: E731
    composed = lambda: st._compose_appearance(slots, images, reference, 0.5, None, stack, 0)  # noqa: E731
    got, want = fused(), composed()
    same = same_bits(got, want, stack)
    visible_share = float(got.count.sum()) / float(H * W * T)
    del got, want
    n = H * W
    unavoidable = (8 + C + (C + 1 if stack else 0)) * n * T + (C + 2 * 4 * C + 4) * n
    res = {"H": H, "W": W, "C": C, "columns": T, "stack": bool(stack), "same_bits": same, "visible_share": visible_share,
           "unavoidable_bytes": int(unavoidable), "fused_peak_bytes": peak_bytes(fused), "composition_peak_bytes": peak_bytes(composed)}
    a, b, ra, rb = legs(fused, composed)
    res["call_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a,
                      "fused_bytes_per_s": unavoidable / (a * 1e-6), "fused_share_of_6.29_TB_s": unavoidable / (a * 1e-6) / HBM}
    # the launch alone: the C function on tables uploaded once and results allocated once
    total, totalsq = (torch.empty((C, H, W), dtype=torch.float32, device=DEV) for _ in range(2))
    count = torch.empty((H, W), dtype=torch.int32, device=DEV)
    warped = torch.empty((T, H, W, C), dtype=torch.uint8, device=DEV) if stack else None
    visible = torch.empty((T, H, W), dtype=torch.bool, device=DEV) if stack else None
    fp, lp = ops.trackstore_slot_addresses(st._chunks, st._lohi, slots)
    ip = np.asarray([i.data_ptr() for i in images], dtype=np.int64)
    tables, (frames_d, lohis_d, images_d) = ops._upload_tables(torch.device(DEV), (fp, lp, ip), ())
    lib = _lib.load()
    args = (frames_d, lohis_d, images_d, T, C, H, W, reference.data_ptr(), 0.5, float("inf"), 0, total.data_ptr(), totalsq.data_ptr(),
            count.data_ptr(), warped.data_ptr() if stack else None, visible.data_ptr() if stack else None)
    fn = lambda: _lib.check(lib.mftx_trackstore_appearance(*args, ops._stream()), "mftx_trackstore_appearance")  # noqa: E731
    k = batch_for(fn)
    t = float(np.median([device_ms(lambda: [fn() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]))
    res["launch_alone_us"] = {"us": t, "share_of_6.29_TB_s": unavoidable / (t * 1e-6) / HBM}
    same_again = bool(torch.equal(count, st.appearance(images, frames, reference=reference).count))
    res["launch_alone_same_count"] = same_again
    del tables
    return res


def pass_store(frames):
    """A tracker pass over ``frames`` frames of the synthetic video with its track store -> (store, the video on the device)."""
    vid = SyntheticVideo(512, 512, n_frames=frames, seed=100)
    conf = config(track_store=True)
    tracker = conf.tracker_class(conf)
    video = []
    for i in range(frames):
        frame = np.ascontiguousarray(vid[i])
        tracker.init(frame) if i == 0 else tracker.track(frame)
        video.append(torch.from_numpy(frame).to(DEV))
    torch.cuda.synchronize()
    return tracker.track_store, video


def smooth_store(H, W, n, C=3):
    st = DenseTrackStore(H, W, device=DEV, frames_per_chunk=n)
    for k, planes in enumerate(smooth_results(H, W, n)):
        st.append(planes, k)
    g = torch.Generator(device="cpu").manual_seed(5)
    video = [torch.randint(0, 256, (H, W, C), generator=g, dtype=torch.uint8).to(DEV) for _ in range(n)]
    return st, video


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_appearance.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_appearance.py measures on the GPU"
    torch.cuda.set_device(0)
    report = {"what": "DenseTrackStore.appearance (mftx_trackstore_appearance) against per-column unpack + warp_backward + torch mask and sums; "
                      "a, b, a, b, a, b in one process, events around batches, medians of %d; microseconds per call" % ROUNDS,
              "device": torch.cuda.get_device_name(0)}
    st, video = pass_store(args.frames)
    for T in sorted({min(50, args.frames), args.frames}):
        for stack in (False, True):
            key = "512x512x3_pass_store_%d_columns%s" % (T, "_stack" if stack else "")
            report[key] = appearance_case(st, list(range(T)), video[:T], video[0], stack)
            print(key, json.dumps(report[key]), flush=True)
    del st, video
    torch.cuda.empty_cache()
    st, video = smooth_store(1080, 1920, 50)
    for stack in (False, True):
        key = "1080x1920x3_smooth_fields_50_columns%s" % ("_stack" if stack else "")
        report[key] = appearance_case(st, list(range(50)), video, video[0], stack)
        print(key, json.dumps(report[key]), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
