#!/usr/bin/env python3
"""What following sparse points costs when the template is chosen per point AND destination frame
(``TrackAtlas.best_query_from``; csrc/trackstore.hip: ts_tracks_best_kernel through ``mftx_trackstore_tracks_from_best``).

The fused call against the composition it replaces -- per-candidate ``atlas.query`` of the located points, ``chain_behind_inverse``
and the key minimum in torch (``TrackAtlas._compose_best_points``, the ``device="cpu"`` path's code on device tensors) -- a, b, a, b,
a, b in ONE process, events around batches, medians.  Timed twice: the whole call (step A, the un-reduced ``mftx_trackstore_locate``
call, included on both sides) and step B alone (both sides given the same step-A rows).  The two results are compared as the GPU
tests compare them: bits where the composition's value is no NaN, NaN-ness elsewhere, ``entry`` equal.

Cases: those of tools/bench_track_atlas_best.py -- 512 x 512, a 50-frame forward pass of 10 start frames on the pass's own stores;
1080 x 1920, 32 templates of seeded smooth fields.  Point sets: the 30-pixel grid given on one frame, the same points spread over (up
to) 50 source frames, and 1 point; columns: all of them and 1.  Step B is also timed for several numbers of columns per workgroup.
On the pass's own stores: the share of point-columns that are fill, and that are visible (occlusion <= 0.5), under ``tracks_from``
and under ``best_tracks_from``.

Writes profiles/track_atlas_points.json.

    python tools/bench_track_atlas_points.py [--out profiles/track_atlas_points.json]
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

from mft_amd import atlas_ops  # noqa: E402
from bench_track_atlas_flow import COLUMNS_1080P, ROUNDS, legs, pass_atlas, smooth_atlas  # noqa: E402
from bench_track_inverse import batch_for, device_ms  # noqa: E402

DEV = "cuda"
THR = 0.5
COLUMNS_PER_BLOCK = (1, 4, 16, 0x7fffffff)            # the last: one workgroup walks all columns
GRID_STEP = 30


def grid_points(H, W):
    ys, xs = np.mgrid[GRID_STEP // 2:H:GRID_STEP, GRID_STEP // 2:W:GRID_STEP]
    return torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)).to(DEV)


def same_rows(got, want):
    nan = torch.isnan(want[0])
    return bool(torch.equal(torch.isnan(got[0]), nan)) and bool(torch.equal(got[0].view(torch.int32)[~nan], want[0].view(torch.int32)[~nan])) \
        and bool(torch.equal(got[1], want[1]))


def points_case(atlas, xy, frame, cols, coverage=False):
    N, T = int(xy.shape[0]), len(cols)
    groups, holders = atlas._point_groups(frame, N, "bench")
    out = (torch.empty((N, T, 4), dtype=torch.float32, device=DEV), torch.empty((N, T), dtype=torch.int32, device=DEV))
    tq, cq = atlas._locate_candidates(xy, groups, holders, THR)
    host_tables = atlas._points_tables(groups, holders, cols, N)

    def composed_call():
        return atlas._compose_best_points(*atlas._locate_candidates(xy, groups, holders, THR), groups, holders, cols, THR, N)

    whole_a, whole_b = (lambda: atlas.best_query_from(xy, frame, cols, THR, out=out)), composed_call
    step_a = lambda: atlas_ops.trackstore_tracks_from_best(tq, cq, *host_tables, (atlas.H, atlas.W), *out, THR)  # noqa: E731
    step_b = lambda: atlas._compose_best_points(tq, cq, groups, holders, cols, THR, N)  # noqa: E731
    got, want = whole_a(), whole_b()
    res = {"H": atlas.H, "W": atlas.W, "entries": len(atlas.entries), "points": N, "source_frames": len(groups), "columns": T,
           "candidates_per_source_frame_min_max": [min(map(len, holders)), max(map(len, holders))], "located_rows": int(tq.shape[0]),
           "same_bits_where_not_nan_nan_where_nan_entry_equal": same_rows(got, want)}
    if coverage:
        old = atlas.tracks_from(xy, frame, cols, THR)
        new = atlas.best_tracks_from(xy, frame, cols, THR)
        with np.errstate(invalid="ignore"):
            res["tracks_from"] = {"fill_share": float(np.isnan(old[0][:, :, 0]).mean()),
                                  "visible_share": float((~np.isnan(old[0][:, :, 0]) & (old[1] <= THR)).mean())}
            res["best_tracks_from"] = {"fill_share": float((~new[2]).mean()), "visible_share": float((new[2] & (new[1] <= THR)).mean())}
    a, b, ra, rb = legs(whole_a, whole_b)
    res["whole_call_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a}
    a, b, ra, rb = legs(step_a, step_b)
    res["step_b_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a}
    loc = lambda: atlas._locate_candidates(xy, groups, holders, THR)  # noqa: E731
    k = batch_for(loc)
    res["step_a_us"] = float(np.median([device_ms(lambda: [loc() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]))
    sweep = {}
    for cpb in COLUMNS_PER_BLOCK:
        if cpb != COLUMNS_PER_BLOCK[-1] and cpb >= T:                                # (as good as "all")
            continue
        fn = lambda: atlas_ops.trackstore_tracks_from_best(tq, cq, *host_tables, (atlas.H, atlas.W), *out, THR, columns_per_block=cpb)  # noqa: E731
        k = batch_for(fn)
        t = [device_ms(lambda: [fn() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]
        sweep["all" if cpb == COLUMNS_PER_BLOCK[-1] else str(cpb)] = float(np.median(t))
    res["fused_step_b_us_by_columns_per_workgroup"] = sweep
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_atlas_points.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_atlas_points.py measures on the GPU"
    torch.cuda.set_device(0)
    report = {"what": "TrackAtlas.best_query_from (mftx_trackstore_locate + mftx_trackstore_tracks_from_best) against the same locate + "
                      "per-candidate query + chaining + the key minimum in torch; a, b, a, b, a, b in one process, events around batches, "
                      "medians of %d; microseconds per call" % ROUNDS,
              "device": torch.cuda.get_device_name(0), "columns_per_workgroup_default": atlas_ops.TRACKSTORE_POINTS_COLUMNS}

    def case(name, *a, **kw):
        report[name] = points_case(*a, **kw)
        print(name, json.dumps(report[name]), flush=True)

    def cases(prefix, atlas, one_frame, one_column, many_frames, coverage):
        xy = grid_points(atlas.H, atlas.W)
        spread = [many_frames[i % len(many_frames)] for i in range(int(xy.shape[0]))]
        for cols_name, cols in (("all_columns", list(atlas.frames)), ("1_column", [one_column])):
            case(f"{prefix}_grid_on_one_frame_{cols_name}", atlas, xy, one_frame, cols, coverage=coverage)
            case(f"{prefix}_grid_over_{len(many_frames)}_source_frames_{cols_name}", atlas, xy, spread, cols, coverage=coverage)
            case(f"{prefix}_1_point_{cols_name}", atlas, xy[len(xy) // 2:len(xy) // 2 + 1], one_frame, cols)

    atlas = pass_atlas(args.frames, args.stride)
    cases("512x512_pass_stores", atlas, args.frames - 1, args.frames - 1, list(atlas.frames)[:50], True)
    del atlas
    torch.cuda.empty_cache()
    atlas = smooth_atlas(1080, 1920, 32, COLUMNS_1080P)
    cases("1080x1920_smooth_fields", atlas, 100, 101, [f for f in atlas.frames if f >= 100][:50], False)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
