"""Torch-tensor front end of the track atlas's per-(pixel, column) read-out (``mftx_trackstore_flow_from_best``), by the contract of
mft_amd/ops.py: device / dtype / contiguity checked, raw device pointers and the current HIP stream passed, ``MftxError`` on a
non-zero return.  The host tables go up through ``ops._upload_tables``; stream ordering is held by
tests/test_gpu_track_atlas_best.py."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import MftxError, check

TRACKSTORE_BEST_COLUMNS = 16             # columns per workgroup of mftx_trackstore_flow_from_best unless the caller says otherwise
TRACKSTORE_BEST_ENTRIES = 256            # candidates per call (8 bits of its key)


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
