#!/usr/bin/env python3
"""What the dense flow between any two frames costs across templates (``TrackAtlas.results_from``; csrc/trackstore.hip:
ts_flow_from_kernel through ``mftx_trackstore_flow_from``).

The fused call against the composition it replaces -- ``atlas.inverse``, per-template ``atlas.query`` of every pixel and the torch
rule of ``DenseTrackStore.results_from`` (``TrackAtlas._compose_results``, the ``device="cpu"`` path's code on device tensors) --
a, b, a, b, a, b in ONE process, events around batches, medians.  Timed twice: the whole call (the inverse included on both
sides) and the second step alone (both sides given the same inverse).  The two results are compared as the GPU tests compare
them: bits where the composition's value is no NaN, NaN-ness elsewhere.

Cases: 512 x 512, a 50-frame forward pass of 10 start frames (every fifth; stand-in weights) on the pass's own stores, from the
last frame to all 50 frames and to the last frame alone; 1080 x 1920, 32 templates of seeded smooth fields that all hold the
source frame and COLUMNS further frames each, to all of those and to one.  Per case and leg: time per call, the bytes the call
cannot avoid -- per pixel a table row and an entry (20 B), per pixel and column 16 B of results, and 4 taps of 8 B where the
pixel is found and its template covers the column -- with the rate they imply against 6.29 TB/s, and the peak bytes allocated.
The fused step is also timed for several numbers of columns per workgroup.

Writes profiles/track_atlas_flow.json.

    python tools/bench_track_atlas_flow.py [--out profiles/track_atlas_flow.json]
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

from mft_amd import ops  # noqa: E402
from mft_amd.multi import MultiTemplateMFT  # noqa: E402
from mft_amd.synth import SyntheticVideo  # noqa: E402
from mft_amd.trackatlas import TrackAtlas  # noqa: E402
from mft_amd.trackstore import DenseTrackStore  # noqa: E402
from bench_track_atlas import config, peak_bytes, run_pass  # noqa: E402
from bench_track_inverse import batch_for, device_ms  # noqa: E402
from bench_track_locate import smooth_results  # noqa: E402

DEV = "cuda"
ROUNDS = 3
HBM = 6.29e12
COLUMNS_1080P = 32
COLUMNS_PER_BLOCK = (1, 4, 16, 64, 0x7fffffff)           # the last: one workgroup walks all columns


def same_results(got, want):
    ok = True
    for g, w in zip(got[:3], want[:3]):
        nan = torch.isnan(w)
        ok = ok and bool(torch.equal(torch.isnan(g), nan)) and bool(torch.equal(g.view(torch.int32)[~nan], w.view(torch.int32)[~nan]))
    return ok


def legs(fa, fb):
    """-> (microseconds per call of a, of b, their (min, max)): a, b, a, b, a, b, events around batches of about 50 ms."""
    na, nb = batch_for(fa), batch_for(fb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(device_ms(lambda: [fa() for _ in range(na)]) * 1e3 / na)
        tb.append(device_ms(lambda: [fb() for _ in range(nb)]) * 1e3 / nb)
    return float(np.median(ta)), float(np.median(tb)), [float(min(ta)), float(max(ta))], [float(min(tb)), float(max(tb))]


def flow_case(atlas, src, cols):
    H, W, T = atlas.H, atlas.W, len(cols)
    out = tuple(torch.empty(s, dtype=torch.float32, device=DEV) for s in ((T, 2, H, W), (T, 1, H, W), (T, 1, H, W)))
    table, _, entry = atlas.inverse(src)
    tables = atlas._flow_tables(cols)

    def composed_call():
        t, _, e = atlas.inverse(src)
        return atlas._compose_results(t, e, cols)

    whole_a, whole_b = (lambda: atlas.results_from(src, cols, out=out)), composed_call
    step_a, step_b = (lambda: ops.trackstore_flow_from(table, entry, *tables, *out)), (lambda: atlas._compose_results(table, entry, cols))
    got, want = whole_a(), whole_b()
    same = same_results(got, want)
    read = int((~torch.isnan(want[0][:, 0])).sum())                                   # pixel-columns that are found and covered
    found = float((entry >= 0).float().mean())
    del want
    n = H * W
    bytes_step = 20 * n + 16 * n * T + 32 * read
    res = {"H": H, "W": W, "entries": len(atlas.entries), "templates": len(atlas._templates()[0]), "columns": T, "source_frame": int(src),
           "same_bits_where_not_nan_and_nan_where_nan": bool(same), "found_share": found, "pixel_columns_read_share": read / float(n * T),
           "unavoidable_bytes_second_step": int(bytes_step),
           "fused_peak_bytes": peak_bytes(lambda: atlas.results_from(src, cols)), "composition_peak_bytes": peak_bytes(whole_b)}
    a, b, ra, rb = legs(whole_a, whole_b)
    res["whole_call_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a}
    a, b, ra, rb = legs(step_a, step_b)
    res["second_step_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a,
                             "fused_bytes_per_s": bytes_step / (a * 1e-6), "fused_share_of_6.29_TB_s": bytes_step / (a * 1e-6) / HBM,
                             "composition_bytes_per_s": bytes_step / (b * 1e-6), "composition_share_of_6.29_TB_s": bytes_step / (b * 1e-6) / HBM}
    sweep = {}
    for cpb in COLUMNS_PER_BLOCK:
        if cpb != COLUMNS_PER_BLOCK[-1] and cpb >= T:                                # (as good as "all")
            continue
        fn = lambda: ops.trackstore_flow_from(table, entry, *tables, *out, columns_per_block=cpb)  # noqa: E731
        k = batch_for(fn)
        t = [device_ms(lambda: [fn() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]
        sweep["all" if cpb == COLUMNS_PER_BLOCK[-1] else str(cpb)] = float(np.median(t))
    res["fused_step_us_by_columns_per_workgroup"] = sweep
    return res


def pass_atlas(frames, stride):
    vid = SyntheticVideo(512, 512, n_frames=frames, seed=100)
    video = [np.ascontiguousarray(vid[i]) for i in range(frames)]
    starts = list(range(0, frames, stride))
    mt = MultiTemplateMFT(config(multi_template_stores=True))
    run_pass(mt, video, starts)
    return TrackAtlas([(s, mt.track_stores[s]) for s in starts])


def smooth_atlas(H, W, n, columns, pool=32):
    """n templates k = 0 .. n - 1 (the identity on their own frame), each holding the source frame 100 and frames 101 .. 100 + columns:
    seeded smooth fields from a pool of ``pool``, combined differently per template."""
    fields = smooth_results(H, W, pool)
    identity = (torch.zeros(2, H, W, device=DEV), torch.zeros(1, H, W, device=DEV), torch.zeros(1, H, W, device=DEV))
    entries = []
    for k in range(n):
        st = DenseTrackStore(H, W, device=DEV, frames_per_chunk=columns + 2)
        st.append(identity, k)
        for j in range(columns + 1):
            st.append(fields[(k + 3 * j) % pool], 100 + j)
        entries.append((k, st))
    return TrackAtlas(entries)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_atlas_flow.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_atlas_flow.py measures on the GPU"
    torch.cuda.set_device(0)
    report = {"what": "TrackAtlas.results_from (mftx_trackstore_flow_from) against inverse + per-template query + the torch rule; a, b, a, b, "
                      "a, b in one process, events around batches, medians of %d; microseconds per call" % ROUNDS,
              "device": torch.cuda.get_device_name(0), "columns_per_workgroup_default": ops.TRACKSTORE_FLOW_COLUMNS}
    atlas = pass_atlas(args.frames, args.stride)
    last = args.frames - 1
    report["512x512_pass_stores_%d_columns" % args.frames] = flow_case(atlas, last, list(atlas.frames))
    report["512x512_pass_stores_1_column"] = flow_case(atlas, last, [last])
    del atlas
    torch.cuda.empty_cache()
    atlas = smooth_atlas(1080, 1920, 32, COLUMNS_1080P)
    report["1080x1920_smooth_fields_%d_columns" % COLUMNS_1080P] = flow_case(atlas, 100, list(range(101, 101 + COLUMNS_1080P)))
    report["1080x1920_smooth_fields_1_column"] = flow_case(atlas, 100, [101])
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
