#!/usr/bin/env python3
"""What the dense flow between any two frames costs when the template is chosen per pixel AND destination frame
(``TrackAtlas.best_results_from``; csrc/trackstore.hip: ts_flow_best_kernel through ``mftx_trackstore_flow_from_best``).

The fused call against the composition it replaces -- per-entry inverse, per-candidate ``atlas.query`` of every pixel,
``chain_behind_inverse`` and the key minimum in torch (``TrackAtlas._compose_best``, the ``device="cpu"`` path's code on device
tensors) -- a, b, a, b, a, b in ONE process, events around batches, medians.  Timed twice: the whole call (the per-entry inverses
included on both sides) and step B alone (both sides given the same inverse planes).  The two results are compared as the GPU
tests compare them: bits where the composition's value is no NaN, NaN-ness elsewhere, ``entry`` equal.

Cases: those of tools/bench_track_atlas_flow.py -- 512 x 512, a 50-frame forward pass of 10 start frames on the pass's own stores,
from the last frame to all 50 frames and to the last frame alone; 1080 x 1920, 32 templates of seeded smooth fields that all
hold the source frame, to 32 further frames and to one.  Per case and leg: time per call, the bytes step B cannot avoid -- per
pixel and column block E x 20 B of inverse rows, per (pixel, column, candidate) that has an answer 4 taps of 8 B, 20 B of results
per pixel-column -- with the rate they imply against 6.29 TB/s, and the peak bytes allocated.  Step B is also timed for several
numbers of columns per workgroup.  On the pass's own stores: the share of pixel-columns that are fill, and that are visible
(occlusion <= 0.5), under ``results_from`` and under ``best_results_from``.

Writes profiles/track_atlas_best.json.

    python tools/bench_track_atlas_best.py [--out profiles/track_atlas_best.json]
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
from bench_track_atlas import peak_bytes  # noqa: E402
from bench_track_atlas_flow import COLUMNS_1080P, COLUMNS_PER_BLOCK, HBM, ROUNDS, legs, pass_atlas, same_results, smooth_atlas  # noqa: E402
from bench_track_inverse import batch_for, device_ms  # noqa: E402

DEV = "cuda"
THR = 0.5


def shares(flow, occl):
    """-> (share of pixel-columns that are fill, share that are visible)."""
    fill = flow[:, 0].contiguous().view(torch.int32) == 0x7fc00000
    return float(fill.float().mean()), float(((occl[:, 0] <= THR) & ~fill).float().mean())


def best_case(atlas, src, cols, coverage=False):
    H, W, T = atlas.H, atlas.W, len(cols)
    n = H * W
    ranks = atlas._holders(src)
    E = len(ranks)
    out = tuple(torch.empty(s, dtype=torch.float32, device=DEV) for s in ((T, 2, H, W), (T, 1, H, W), (T, 1, H, W)))
    entry = torch.empty((T, H, W), dtype=torch.int32, device=DEV)
    tables, cells = atlas._entry_inverses(src, ranks, THR)
    host_tables = atlas._best_tables(ranks, cols)

    def composed_call():
        return atlas._compose_best(*atlas._entry_inverses(src, ranks, THR), ranks, cols, THR)

    whole_a, whole_b = (lambda: atlas.best_results_from(src, cols, out=out)), composed_call
    step_a = lambda: atlas_ops.trackstore_flow_from_best(tables, cells, *host_tables, *out, entry, THR)  # noqa: E731
    step_b = lambda: atlas._compose_best(tables, cells, ranks, cols, THR)  # noqa: E731
    got, want = whole_a(), whole_b()
    same = same_results(got, want) and bool(torch.equal(got[3], want[3]))
    answers = sum(int((cells[k] >= 0).sum()) * int(np.sum(atlas.covered(atlas.entries[r][0], cols))) for k, r in enumerate(ranks))
    col_blocks = -(-T // atlas_ops.TRACKSTORE_BEST_COLUMNS)
    bytes_step = 20 * E * n * col_blocks + 32 * answers + 20 * n * T
    res = {"H": H, "W": W, "entries": len(atlas.entries), "candidates": E, "columns": T, "source_frame": int(src),
           "same_bits_where_not_nan_nan_where_nan_entry_equal": bool(same), "answers_share_of_pixel_column_candidates": answers / float(n * T * E),
           "unavoidable_bytes_step_b": int(bytes_step), "inverse_planes_bytes": int(tables.numel() * 4 + cells.numel() * 4)}
    if coverage:
        old = atlas.results_from(src, cols)
        f0, v0 = shares(old[0], old[1])
        f1, v1 = shares(got[0], got[1])
        res["results_from"] = {"fill_share": f0, "visible_share": v0}
        res["best_results_from"] = {"fill_share": f1, "visible_share": v1}
        del old
    del got, want
    res["fused_peak_bytes"] = peak_bytes(lambda: atlas.best_results_from(src, cols))
    res["composition_peak_bytes"] = peak_bytes(whole_b)
    a, b, ra, rb = legs(whole_a, whole_b)
    res["whole_call_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a}
    a, b, ra, rb = legs(step_a, step_b)
    res["step_b_us"] = {"fused": a, "composition": b, "fused_min_max": ra, "composition_min_max": rb, "composition_over_fused": b / a,
                        "fused_bytes_per_s": bytes_step / (a * 1e-6), "fused_share_of_6.29_TB_s": bytes_step / (a * 1e-6) / HBM}
    inv = lambda: atlas._entry_inverses(src, ranks, THR)  # noqa: E731
    k = batch_for(inv)
    res["step_a_us"] = float(np.median([device_ms(lambda: [inv() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]))
    sweep = {}
    for cpb in COLUMNS_PER_BLOCK:
        if cpb != COLUMNS_PER_BLOCK[-1] and cpb >= T:                                # (as good as "all")
            continue
        fn = lambda: atlas_ops.trackstore_flow_from_best(tables, cells, *host_tables, *out, entry, THR, columns_per_block=cpb)  # noqa: E731
        k = batch_for(fn)
        t = [device_ms(lambda: [fn() for _ in range(k)]) * 1e3 / k for _ in range(ROUNDS)]
        sweep["all" if cpb == COLUMNS_PER_BLOCK[-1] else str(cpb)] = float(np.median(t))
    res["fused_step_b_us_by_columns_per_workgroup"] = sweep
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "track_atlas_best.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_atlas_best.py measures on the GPU"
    torch.cuda.set_device(0)
    report = {"what": "TrackAtlas.best_results_from (mftx_trackstore_flow_from_best) against per-entry inverse + per-candidate query + "
                      "chaining + the key minimum in torch; a, b, a, b, a, b in one process, events around batches, medians of %d; "
                      "microseconds per call" % ROUNDS,
              "device": torch.cuda.get_device_name(0), "columns_per_workgroup_default": atlas_ops.TRACKSTORE_BEST_COLUMNS}

    def case(name, *a, **kw):
        report[name] = best_case(*a, **kw)
        print(name, json.dumps(report[name]), flush=True)

    atlas = pass_atlas(args.frames, args.stride)
    last = args.frames - 1
    case("512x512_pass_stores_%d_columns" % args.frames, atlas, last, list(atlas.frames), coverage=True)
    case("512x512_pass_stores_1_column", atlas, last, [last], coverage=True)
    case("512x512_pass_stores_first_frame_column", atlas, last, [0], coverage=True)
    del atlas
    torch.cuda.empty_cache()
    atlas = smooth_atlas(1080, 1920, 32, COLUMNS_1080P)
    case("1080x1920_smooth_fields_%d_columns" % COLUMNS_1080P, atlas, 100, list(range(101, 101 + COLUMNS_1080P)))
    case("1080x1920_smooth_fields_1_column", atlas, 100, [101])
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
