"""Torch-tensor front end of the track atlas's per-(pixel, column) and per-(point, column) read-outs
(``mftx_trackstore_flow_from_best``, ``mftx_trackstore_tracks_from_best``) and of the track store's read-out of the video along its
tracks (``mftx_trackstore_appearance``), by the contract of mft_amd/ops.py: device / dtype / contiguity checked, raw device pointers
and the current HIP stream passed, ``MftxError`` on a non-zero return.  The host tables go up through ``ops._upload_tables``; stream
ordering is held by tests/test_gpu_track_atlas_best.py, tests/test_gpu_track_atlas_points.py and tests/test_gpu_track_appearance.py."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import MftxError, check

TRACKSTORE_BEST_COLUMNS = 16             # columns per workgroup of mftx_trackstore_flow_from_best unless the caller says otherwise
TRACKSTORE_BEST_ENTRIES = 256            # candidates per call (8 bits of its key)
TRACKSTORE_POINTS_COLUMNS = 16           # columns per workgroup of mftx_trackstore_tracks_from_best unless the caller says otherwise
TRACKSTORE_POINTS_TILE = 64              # points per tile of that kernel: a wave's lanes


def trackstore_flow_from_best(tables, cells, rank_of, row_of, frame_ptrs, lohi_ptrs, flow, occl, sigma, entry,
                              occlusion_threshold=0.5, columns_per_block=0):
    """The per-entry inverse planes of ONE video frame followed densely over T columns, the entry chosen per pixel and column, in one
    call (``mftx_trackstore_flow_from_best``).  tables (float32 device [E,H,W,4]) and cells (int32 device [E,H,W]): candidate k's
    own dense inverse of the frame (``trackstore_invert``, or ``trackstore_invert_atlas`` with one entry per plane); rank_of / row_of:
    E HOST integers each, candidate -> rank (what ``entry`` reports, 0 .. 255) and candidate -> row; frame_ptrs / lohi_ptrs: HOST
    int64 [R, T] as for ``ops.trackstore_flow_from``, 0 where that row's template does not cover the column.  ``flow`` (float32
    device [T,2,H,W]), ``occl``, ``sigma`` ([T,1,H,W]) and ``entry`` (int32 device [T,H,W]) receive per pixel and column the chained
    result and the rank of the candidate with the smallest key (occluded, chained sigma, rank) -- a NaN occlusion counts as
    occluded, a NaN sigma sorts behind +inf -- and NaN, 1, +inf, -1 where no candidate found the pixel on a template that covers
    the column.  E may be 0: everything is fill.  ``columns_per_block``: the columns a workgroup walks (0:
    TRACKSTORE_BEST_COLUMNS); the results do not depend on it.  The tables go up through one pinned buffer; no host
    synchronisation.  Returns (flow, occl, sigma, entry)."""
    lib = _lib.load()
    rank_of = np.asarray(rank_of, dtype=np.int64).reshape(-1)
    row_of = np.asarray(row_of, dtype=np.int64).reshape(-1)
    frame_ptrs, lohi_ptrs = np.asarray(frame_ptrs, dtype=np.int64), np.asarray(lohi_ptrs, dtype=np.int64)
    if tables.dim() != 4 or int(tables.shape[3]) != 4 or tuple(cells.shape) != tuple(tables.shape[:3]):
        raise MftxError("trackstore_flow_from_best: tables must be [E, H, W, 4], cells [E, H, W]")
    E, H, W = (int(s) for s in tables.shape[:3])
    if E > TRACKSTORE_BEST_ENTRIES:
        raise MftxError(f"trackstore_flow_from_best: more than {TRACKSTORE_BEST_ENTRIES} candidates")
    if frame_ptrs.ndim != 2 or frame_ptrs.shape != lohi_ptrs.shape or ((frame_ptrs == 0) != (lohi_ptrs == 0)).any():
        raise MftxError("trackstore_flow_from_best: frame_ptrs and lohi_ptrs must be [R, T], zero in the same places")
    R, T = (int(s) for s in frame_ptrs.shape)
    if int(rank_of.shape[0]) != E or int(row_of.shape[0]) != E:
        raise MftxError("trackstore_flow_from_best: rank_of and row_of must name a rank and a row for each of the E candidates")
    if E and (R < 1 or row_of.min() < 0 or row_of.max() >= R or rank_of.min() < 0 or rank_of.max() >= TRACKSTORE_BEST_ENTRIES):
        raise MftxError(f"trackstore_flow_from_best: rows must be 0 .. R - 1 with R >= 1, ranks 0 .. {TRACKSTORE_BEST_ENTRIES - 1}")
    if tuple(flow.shape) != (T, 2, H, W) or tuple(occl.shape) != (T, 1, H, W) or tuple(sigma.shape) != (T, 1, H, W) \
            or tuple(entry.shape) != (T, H, W):
        raise MftxError("trackstore_flow_from_best: flow must be [T, 2, H, W], occl and sigma [T, 1, H, W], entry [T, H, W]")
    tp, cp = ops._chk(tables, "tables"), ops._chk(cells, "cells", torch.int32)
    fp, op, sp, ep = ops._chk(flow, "flow"), ops._chk(occl, "occl"), ops._chk(sigma, "sigma"), ops._chk(entry, "entry", torch.int32)
    if T == 0:
        return flow, occl, sigma, entry
    if E == 0:          # (empty tensors have no storage to point at, and there are no tables to send)
        check(lib.mftx_trackstore_flow_from_best(None, None, None, None, None, None, 0, R, T, H, W, float(occlusion_threshold),
                                                 int(columns_per_block), fp, op, sp, ep, ops._stream()), "mftx_trackstore_flow_from_best")
        return flow, occl, sigma, entry
    up, (frames, lohis, ranks, rows) = ops._upload_tables(tables.device, (frame_ptrs.reshape(-1), lohi_ptrs.reshape(-1)), (rank_of, row_of))
    check(lib.mftx_trackstore_flow_from_best(tp, cp, ranks, rows, frames, lohis, E, R, T, H, W, float(occlusion_threshold),
                                             int(columns_per_block), fp, op, sp, ep, ops._stream()), "mftx_trackstore_flow_from_best")
    return flow, occl, sigma, entry


def points_tables(group_sizes, group_candidates):
    """The tile and group tables of ``mftx_trackstore_tracks_from_best`` for points sorted by source frame: group g has
    ``group_sizes[g]`` points (>= 1) and ``group_candidates[g]`` candidates; step A's rows run group after group and, within a group,
    candidate after candidate -> (tiles [n_tiles, 2] = (group, first point within it), groups [G, 5] = (first row, points, first
    sorted point, first candidate, one past the last candidate), Q, C) as int64 host arrays and two integers."""
    sizes = np.asarray(group_sizes, dtype=np.int64).reshape(-1)
    cands = np.asarray(group_candidates, dtype=np.int64).reshape(-1)
    if sizes.shape != cands.shape or (sizes < 1).any() or (cands < 0).any():
        raise MftxError("points_tables: a size >= 1 and a candidate count >= 0 per group")
    rows, cand0 = np.concatenate([[0], np.cumsum(sizes * cands)]), np.concatenate([[0], np.cumsum(cands)])
    point0 = np.concatenate([[0], np.cumsum(sizes)])
    groups = np.stack([rows[:-1], sizes, point0[:-1], cand0[:-1], cand0[1:]], axis=1).reshape(-1, 5)
    tiles = np.asarray([(g, first) for g, n in enumerate(sizes) for first in range(0, int(n), TRACKSTORE_POINTS_TILE)],
                       dtype=np.int64).reshape(-1, 2)
    return tiles, groups, int(rows[-1]), int(cand0[-1])


def trackstore_tracks_from_best(located, cells, group_sizes, group_candidates, rank_of, row_of, order, frame_ptrs, lohi_ptrs, frame_size,
                                table, entry, occlusion_threshold=0.5, columns_per_block=0):
    """Points given on any number of source frames followed over T columns, the candidate chosen per point and column, in one call
    (``mftx_trackstore_tracks_from_best``).  The N points are SORTED by source frame into G groups of ``group_sizes`` points;
    group g has ``group_candidates[g]`` candidates.  located (float32 device [Q, 4]) and cells (int32 device [Q]): the un-reduced
    rows of ``ops.trackstore_locate_frames`` with the points repeated per candidate -- group after group, within a group candidate
    after candidate; rank_of / row_of: HOST integers per candidate of every group, in that order; order: N HOST integers, sorted
    point -> row of the results; frame_ptrs / lohi_ptrs: HOST int64 [R, T] as for ``ops.trackstore_flow_from``; frame_size: (H, W) of
    the stored frames.  ``table`` (float32
    device [N, T, 4]) and ``entry`` (int32 device [N, T]) receive per point and column (x, y, chained occlusion, chained sigma) and
    the rank of the candidate with the smallest key of ``trackstore_flow_from_best``, and NaN, NaN, 1, +inf, -1 where no candidate
    found the point on a template that covers the column.  A group may have no candidates: its rows are fill.
    ``columns_per_block``: the columns a workgroup walks (0: TRACKSTORE_POINTS_COLUMNS); the results do not depend on it.  The
    tables go up through one pinned buffer; no host synchronisation.  Returns (table, entry)."""
    lib = _lib.load()
    name = "trackstore_tracks_from_best"
    tiles, groups, Q, C = points_tables(group_sizes, group_candidates)
    rank_of = np.asarray(rank_of, dtype=np.int64).reshape(-1)
    row_of = np.asarray(row_of, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    frame_ptrs, lohi_ptrs = np.asarray(frame_ptrs, dtype=np.int64), np.asarray(lohi_ptrs, dtype=np.int64)
    if table.dim() != 3 or int(table.shape[2]) != 4 or tuple(entry.shape) != tuple(table.shape[:2]):
        raise MftxError(f"{name}: table must be [N, T, 4], entry [N, T]")
    N, T = int(table.shape[0]), int(table.shape[1])
    G = int(groups.shape[0])
    if int(groups[:, 1].sum()) != N or int(order.shape[0]) != N or (N and not np.array_equal(np.sort(order), np.arange(N))):
        raise MftxError(f"{name}: the groups must hold the N points, and order must name each of the N rows once")
    if tuple(located.shape) != (Q, 4) or tuple(cells.shape) != (Q,):
        raise MftxError(f"{name}: located must be [Q, 4] and cells [Q], Q = {Q} rows of the groups' candidates")
    H, W = (int(s) for s in frame_size)
    most = int((groups[:, 4] - groups[:, 3]).max()) if G else 0
    if most > TRACKSTORE_BEST_ENTRIES:
        raise MftxError(f"{name}: more than {TRACKSTORE_BEST_ENTRIES} candidates in a group")
    if frame_ptrs.ndim != 2 or frame_ptrs.shape != lohi_ptrs.shape or ((frame_ptrs == 0) != (lohi_ptrs == 0)).any():
        raise MftxError(f"{name}: frame_ptrs and lohi_ptrs must be [R, T], zero in the same places")
    R = int(frame_ptrs.shape[0])
    if int(frame_ptrs.shape[1]) != T:
        raise MftxError(f"{name}: frame_ptrs and lohi_ptrs must have the table's {T} columns")
    if int(rank_of.shape[0]) != C or int(row_of.shape[0]) != C:
        raise MftxError(f"{name}: rank_of and row_of must name a rank and a row for each of the {C} candidates")
    if C and (R < 1 or row_of.min() < 0 or row_of.max() >= R or rank_of.min() < 0 or rank_of.max() >= TRACKSTORE_BEST_ENTRIES):
        raise MftxError(f"{name}: rows must be 0 .. R - 1 with R >= 1, ranks 0 .. {TRACKSTORE_BEST_ENTRIES - 1}")
    if Q > 0x7fffffff:
        raise MftxError(f"{name}: more than 2^31 - 1 rows")
    lp, cp = ops._chk(located, "located"), ops._chk(cells, "cells", torch.int32)
    tp, ep = ops._chk(table, "table"), ops._chk(entry, "entry", torch.int32)
    if N == 0 or T == 0:          # (empty tensors have no storage to point at)
        return table, entry
    small = (tiles.reshape(-1), groups.reshape(-1), order) + ((rank_of, row_of) if C else ())
    up, addr = ops._upload_tables(table.device, (frame_ptrs.reshape(-1), lohi_ptrs.reshape(-1)) if C else (), small)
    if C:
        frames, lohis, tl, gr, od, ranks, rows = addr
    else:           # (no candidates anywhere: nothing but the tiles and the results is looked at)
        (tl, gr, od), frames, lohis, ranks, rows, lp, cp = addr, None, None, None, None, None, None
    check(lib.mftx_trackstore_tracks_from_best(lp, cp, tl, gr, ranks, rows, od, frames, lohis, int(tiles.shape[0]), G, C, most, Q, N, R, T,
                                               H, W, float(occlusion_threshold), int(columns_per_block), tp, ep, ops._stream()),
          "mftx_trackstore_tracks_from_best")
    return table, entry


def trackstore_appearance(frame_ptrs, lohi_ptrs, images, reference, sum, sumsq, count, warped=None, visible=None,
                          occlusion_threshold=0.5, sigma_max=None, fill=0):
    """The video sampled along every track of a store and reduced over T columns, in one call (``mftx_trackstore_appearance``).
    frame_ptrs / lohi_ptrs: HOST int64 [T], the packed frame and lohi table of each column (``ops.trackstore_slot_addresses``);
    images: ONE uint8 device tensor [T, H, W, C] or a sequence of T uint8 device tensors [H, W, C], C = 1 .. 4, column k's video frame;
    reference: a uint8 device tensor [H, W, C] or None (= 0).  ``sum`` / ``sumsq`` (float32 device [C, H, W]) and ``count`` (int32
    device [H, W]) receive, per template pixel, the float32 sums over the columns in order of d = sample - reference and d * d and
    the number of columns where the pixel is visible: occlusion <= ``occlusion_threshold``, sigma <= ``sigma_max`` (None: +inf) and
    the position inside the frame.  ``warped`` (uint8 device [T, H, W, C]) and ``visible`` (bool device [T, H, W]), each of
    them or None: the per-column stack, ``fill`` where not visible.  T may be 0: sums and count are zeroed.  The tables go up
    through one pinned buffer; no host synchronisation.  Returns (sum, sumsq, count, warped, visible)."""
    lib = _lib.load()
    name = "trackstore_appearance"
    frame_ptrs = np.asarray(frame_ptrs, dtype=np.int64).reshape(-1)
    lohi_ptrs = np.asarray(lohi_ptrs, dtype=np.int64).reshape(-1)
    T = int(frame_ptrs.shape[0])
    if sum.dim() != 3 or tuple(sumsq.shape) != tuple(sum.shape) or tuple(count.shape) != tuple(sum.shape[1:]):
        raise MftxError(f"{name}: sum and sumsq must be [C, H, W], count [H, W]")
    C, H, W = (int(s) for s in sum.shape)
    if int(lohi_ptrs.shape[0]) != T or (T and ((frame_ptrs == 0).any() or (lohi_ptrs == 0).any())):
        raise MftxError(f"{name}: frame_ptrs and lohi_ptrs must name a stored frame for each of the T columns")
    if isinstance(images, torch.Tensor):
        if tuple(images.shape) != (T, H, W, C):
            raise MftxError(f"{name}: images must be [T, H, W, C] = [{T}, {H}, {W}, {C}]")
        first = ops._chk(images, "images", torch.uint8)
        image_ptrs = first + np.arange(T, dtype=np.int64) * (H * W * C)
    else:
        images = list(images)
        if len(images) != T or any(not isinstance(i, torch.Tensor) or tuple(i.shape) != (H, W, C) for i in images):
            raise MftxError(f"{name}: images must be {T} tensors [H, W, C] = [{H}, {W}, {C}]")
        image_ptrs = np.asarray([ops._chk(i, "images", torch.uint8) for i in images], dtype=np.int64)
    if reference is not None and tuple(reference.shape) != (H, W, C):
        raise MftxError(f"{name}: reference must be [H, W, C] = [{H}, {W}, {C}]")
    if (warped is not None and tuple(warped.shape) != (T, H, W, C)) or (visible is not None and tuple(visible.shape) != (T, H, W)):
        raise MftxError(f"{name}: warped must be [T, H, W, C], visible [T, H, W]")
    if not 0 <= int(fill) <= 255:
        raise MftxError(f"{name}: fill must be 0 .. 255")
    rp = None if reference is None else ops._chk(reference, "reference", torch.uint8)
    sp, qp, cp = ops._chk(sum, "sum"), ops._chk(sumsq, "sumsq"), ops._chk(count, "count", torch.int32)
    wp = None if warped is None else ops._chk(warped, "warped", torch.uint8)
    vp = None if visible is None else ops._chk(visible, "visible", torch.bool)
    if T == 0:          # (nothing to send; the sums over no columns)
        sum.zero_(), sumsq.zero_(), count.zero_()
        return sum, sumsq, count, warped, visible
    up, (frames, lohis, imgs) = ops._upload_tables(sum.device, (frame_ptrs, lohi_ptrs, image_ptrs), ())
    smax = float("inf") if sigma_max is None else float(sigma_max)
    check(lib.mftx_trackstore_appearance(frames, lohis, imgs, T, C, H, W, rp, float(occlusion_threshold), smax, int(fill), sp, qp, cp, wp, vp,
                                         ops._stream()), "mftx_trackstore_appearance")
    return sum, sumsq, count, warped, visible
