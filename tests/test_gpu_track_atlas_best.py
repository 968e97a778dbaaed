"""``TrackAtlas.best_results_from`` on the device (csrc/trackstore.hip: ts_flow_best_kernel through
``atlas_ops.trackstore_flow_from_best``) against the composition it fuses -- ``TrackAtlas._compose_best`` on device tensors: per-entry
inverse, per-template ``atlas.query``, ``chain_behind_inverse`` and the key minimum in torch -- bit for bit wherever the expected
value is no NaN and NaN exactly where it is one; against the host atlas wherever the choice is unambiguous; through a
``MultiTemplateMFT`` pass; behind a stalled stream; and ``DenseTrackStore.results_from`` on a device store against its composition."""
import numpy as np
import pytest
import torch

import stream_catalog as cat
import stream_harness as sh
import test_track_atlas as host
import test_gpu_track_atlas as ga
import test_track_atlas_best as hb
from test_gpu_streams_ops import run_behind_stall
from test_gpu_track_atlas_flow import assert_all_fill, assert_same, bits, case_atlas
from test_track_atlas_flow import INF_BITS, NAN_BITS, ONE_BITS
from test_track_locate import const_planes, field, make_store, shifted_out_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def composition(atlas, src, cols, thr=0.5):
    """The definition on device tensors -> (flow, occlusion, sigma, entry, template)."""
    ranks = atlas._holders(src)
    flow, occl, sigma, entry = atlas._compose_best(*atlas._entry_inverses(src, ranks, thr), ranks, cols, thr)
    tmpl_of = torch.tensor([f for f, _ in atlas.entries], dtype=torch.int32, device=DEV)
    template = torch.where(entry >= 0, tmpl_of[entry.clamp(min=0).long()], torch.full_like(entry, -1))
    return flow.contiguous(), occl.contiguous(), sigma.contiguous(), entry.contiguous(), template


def same(got, want):
    """``assert_same`` of the three planes (bits where the expected value is no NaN, NaN-ness elsewhere); entry and template equal."""
    assert got[3].dtype == torch.int32 and got[3].is_cuda and torch.equal(got[3], want[3]), int((got[3] != want[3]).sum())
    assert_same((got[0], got[1], got[2], got[3] >= 0, got[4]), (want[0], want[1], want[2], want[3] >= 0, want[4]))


def columns(atlas, T):
    return [atlas.frames[(3 * i + i // 4) % len(atlas.frames)] for i in range(T)]     # repeats, no order


# ---- 1. bitwise against the composition on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one template", "a template each"])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("H,W", [(2, 2), (2, 70), (9, 34), (24, 40), (37, 53)])
def test_best_results_from_is_the_composition_bitwise(H, W, T, n, kind):
    from mft_amd import atlas_ops
    assert T <= 5 or T == atlas_ops.TRACKSTORE_BEST_COLUMNS + 1                       # one more than a workgroup walks
    atlas = case_atlas(H, W, n, kind)                                                 # (candidates are walked one at a time: n = 2 is one more)
    cols = columns(atlas, T)
    for src in (1, 2):
        assert len(atlas._holders(src)) == n
        got = atlas.best_results_from(src, cols)
        assert got[0].shape == (T, 2, H, W) and got[1].shape == (T, 1, H, W) and got[2].shape == (T, 1, H, W)
        assert got[3].shape == (T, H, W) and got[4].shape == (T, H, W)
        same(got, composition(atlas, src, cols))
    if n == 5 and T == 17 and kind == "a template each" and (H, W) in ((9, 34), (24, 40), (37, 53)):
        e = atlas.best_results_from(1, cols)[3].reshape(T, -1)
        won = [int((e == k).sum()) for k in range(5)]
        print(f"{H}x{W}: candidates win {won} pixel-columns from frame 1, {int((e < 0).sum())} are fill")
        assert sum(w > 0 for w in won) >= 3                                           # the winners do interleave
        row = e[:, :64 * ((H * W) // 64)].reshape(T, -1, 64)
        assert (row.max(dim=2).values != row.min(dim=2).values).any()                 # ... within a wave's 64 pixels
        assert (e.max(dim=0).values != e.min(dim=0).values).any()                     # ... and across the columns of one pixel


def test_the_three_template_atlas():
    for H, W in ((13, 21), (24, 40)):
        atlas = hb.three_templates(H, W, 1.5, device=DEV)
        for src in (1, 2, 3):
            for cols in (atlas.frames, [3, 0, 0, 2, 1]):
                same(atlas.best_results_from(src, cols), composition(atlas, src, cols))
        old = atlas.results_from(2)
        assert_all_fill(old[0][0:2], old[1][0:2], old[2][0:2])
        e = atlas.best_results_from(2)[3]
        assert float((e < 0).float().mean()) < 0.10 and all(int((e == r).sum()) > 0 for r in range(3))
        assert (e.reshape(4, -1).max(dim=0).values != e.reshape(4, -1).min(dim=0).values).any()


# ---- 2. stores of three chunks, a joined template with uncovered columns inside a column block -----------------------------------
def test_three_chunks_and_a_joined_template():
    from mft_amd import TrackAtlas
    H, W = 24, 40
    fwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 6, 7, 8, 9)}, device=DEV, frames_per_chunk=2)
    bwd = make_store(H, W, {f: (const_planes(H, W) if f == 5 else field(f, H, W, 1.5)) for f in (5, 4, 3, 2, 1)}, device=DEV, frames_per_chunk=2)
    other = make_store(H, W, {11: const_planes(H, W), 10: field(10, H, W, 1.5), 7: field(17, H, W, 5.0)}, device=DEV, frames_per_chunk=2)
    assert len(fwd._chunks) == 3 and len(bwd._chunks) == 3 and len(other._chunks) == 2
    atlas = TrackAtlas([(5, fwd), (5, bwd), (11, other)])
    cols = [1, 9, 10, 2, 8, 11, 3, 7, 10, 4, 6, 11, 5, 12, 7, 1, 9, 11, 10, 2]        # 10, 11 (and 12): not covered by template 5
    for src in (7, 3, 5):
        got = atlas.best_results_from(src, cols)
        same(got, composition(atlas, src, cols))
        if src == 7:
            t = got[4]
            print(f"from frame 7: template 5 wins {int((t == 5).sum())} pixel-columns, template 11 {int((t == 11).sum())}, {int((t < 0).sum())} fill")
            assert (t[1] == 5).any() and (t[1] != 11).all()                            # frame 9: template 5 alone covers it
            assert (t[2] == 11).any() and (t[2] != 5).all()                            # frame 10: template 11 alone
            assert (t[7] == 5).any() and (t[7] == 11).any()                            # frame 7: both, interleaved
            assert (got[3][13] == -1).all() and (bits(got[0][13]) == NAN_BITS).all()   # frame 12: nobody's


# ---- 3. special values -------------------------------------------------------------------------------------------------------
def test_nan_and_inf_come_out_as_the_composition_has_them():
    from mft_amd import TrackAtlas
    s0, s1 = host.two_template_stores(host.AH, host.AW, device=DEV, amp=1.5)
    host.with_sigma_range(s0, 0.5, float("inf"))          # template 0's frame 1: sigma +inf wherever its word is not 0 (NaN where it is)
    host.with_sigma_range(s1, float("nan"))               # template 1's own frame: sigma NaN
    atlas = TrackAtlas([(0, s0), (1, s1)])
    seen_inf = seen_nan = 0
    for src in (1, 2):
        got = atlas.best_results_from(src)
        want = composition(atlas, src, atlas.frames)
        same(got, want)
        read = want[3] >= 0
        seen_inf += int(torch.isposinf(want[2][:, 0][read]).sum())
        seen_nan += int(torch.isnan(want[2][:, 0][read]).sum())
    print(f"sigma of answered pixel-columns: {seen_inf} +inf, {seen_nan} NaN")
    assert seen_inf > 0 and seen_nan > 0


def test_a_source_that_nothing_maps_into():
    from mft_amd import TrackAtlas
    H, W = 24, 40
    st = make_store(H, W, {0: const_planes(H, W), 7: shifted_out_planes(H, W), 2: field(1, H, W, 1.5)}, device=DEV)
    flow, occl, sigma, entry, template = TrackAtlas([(0, st)]).best_results_from(7)
    assert flow.shape == (3, 2, H, W) and (entry == -1).all() and (template == -1).all()
    assert_all_fill(flow, occl, sigma)


# ---- 4. reproducibility, bounds, the columns a workgroup walks ------------------------------------------------------------------
def test_same_bits_every_time_nothing_else_written_whatever_the_column_blocks():
    from mft_amd import atlas_ops
    H, W, T = 37, 53, 21
    atlas = case_atlas(H, W, 5, "a template each")
    cols = columns(atlas, T)
    want = composition(atlas, 2, cols)
    first = atlas.best_results_from(2, cols)
    same(first, want)
    for _ in range(4):
        again = atlas.best_results_from(2, cols)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, first))
    ranks = atlas._holders(2)
    tables, cells = atlas._entry_inverses(2, ranks, 0.5)
    host_tables = atlas._best_tables(ranks, cols)
    for cpb in (1, 2, 0, T):                                                          # a tuning choice, not a result
        big = [torch.full((T + 2, c, H, W), -7.0, device=DEV) for c in (2, 1, 1)] + [torch.full((T + 2, H, W), -7, dtype=torch.int32, device=DEV)]
        atlas_ops.trackstore_flow_from_best(tables, cells, *host_tables, *(b[1:T + 1] for b in big), columns_per_block=cpb)
        assert all(torch.equal(bits(b[1:T + 1]), bits(f)) for b, f in zip(big, first)), cpb
        assert all((b[0] == -7).all() and (b[T + 1] == -7).all() for b in big), cpb
    with pytest.raises(ValueError):
        atlas.best_results_from(2, cols, out=(first[0], first[1], first[2].cpu()))
    with pytest.raises(KeyError):
        atlas.best_results_from(99, cols)
    # no candidates at all: everything is fill
    out = (torch.full((2, 2, H, W), -7.0, device=DEV), torch.full((2, 1, H, W), -7.0, device=DEV), torch.full((2, 1, H, W), -7.0, device=DEV),
           torch.full((2, H, W), -7, dtype=torch.int32, device=DEV))
    atlas_ops.trackstore_flow_from_best(tables[:0], cells[:0], [], [], np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64), *out)
    assert_all_fill(*out[:3])
    assert (out[3] == -1).all()


# ---- 5. against the host atlas -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,amp", hb.HOST_CASES)
def test_device_and_host_atlas_agree_where_the_choice_is_unambiguous(H, W, amp):
    """``entry`` equal wherever the host's own candidates leave no doubt (tests/test_track_atlas_best.py: ``ambiguous``), and there
    flow, occlusion and sigma within what tests/test_gpu_track_atlas_flow.py::test_device_and_host_atlas_agree accepts between the
    device sampler and torch's: 1e-5 px, 1e-6, 1e-6.  The fill is the same set of pixel-columns: the inverses agree bit for bit."""
    cpu, want, amb, answered = hb.host_case(H, W, amp)
    dev = hb.three_templates(H, W, amp, device=DEV)
    got = [t.cpu() for t in dev.best_results_from(2)]
    share = amb.sum() / answered.sum()
    assert share <= hb.AMBIGUOUS_CAP
    clear = torch.from_numpy((answered & ~amb).reshape(want[3].shape))
    assert torch.equal(got[3] < 0, want[3] < 0) and torch.equal(got[3] < 0, torch.from_numpy(~answered).reshape(want[3].shape))
    assert torch.equal(got[3][clear], want[3][clear]) and torch.equal(got[4][clear], want[4][clear])
    other = int((got[3] != want[3]).sum())
    print(f"{H}x{W} amp {amp}: {int(amb.sum())} of {int(answered.sum())} answered pixel-columns ambiguous ({share:.3%}); "
          f"another winner than the host's on {other}")
    for name, g, w, tol in (("flow", got[0], want[0], 1e-5), ("occlusion", got[1], want[1], 1e-6), ("sigma", got[2], want[2], 1e-6)):
        m = clear[:, None].expand_as(w)
        err = float((g[m] - w[m]).abs().max())
        print(f"{H}x{W} amp {amp} {name}: device and host differ by at most {err:.3g} (accepted: {tol:g})")
        assert err <= tol
        fill = (want[3] < 0)[:, None].expand_as(w)
        assert torch.equal(bits(g)[fill], bits(w)[fill])


# ---- 6. through the engine ---------------------------------------------------------------------------------------------------
def test_backward_columns_from_a_mid_video_template_frame_through_the_engine():
    from mft_amd import TrackAtlas
    from mft_amd.results import FlowOUTrackingResult
    fwd, bwd = (p[0] for p in ga.passes_with_stores(1))
    atlas = TrackAtlas.from_passes(fwd, bwd)
    mid = 5                                                # a template of the forward pass: its store holds frames 5 .. 11 only
    assert [t for t, _ in atlas.entries] == [0, 3, 5, 7, 11] and atlas.frames == list(range(ga.N_FRAMES))
    assert atlas._holders(mid) == [0, 1, 2, 3, 4] and atlas.covered(mid)[:mid] == [False] * mid
    old = atlas.results_from(mid)
    assert (old[4] == mid).all()                           # sigma 0 on its own frame: template 5 wins every pixel ...
    assert_all_fill(old[0][:mid], old[1][:mid], old[2][:mid])                          # ... and every backward column is fill
    got = atlas.best_results_from(mid)
    same(got, composition(atlas, mid, atlas.frames))
    flow, occl, sigma, entry, template = got
    # answered exactly where some candidate whose template covers the column finds the pixel
    finds = {s: st.inverse(mid)[1] >= 0 for s, st in atlas.entries}
    for t, f in enumerate(atlas.frames):
        expect = torch.zeros_like(entry[t], dtype=torch.bool)
        for s in finds:
            if atlas.covered(s, [f])[0]:
                expect |= finds[s]
        assert torch.equal(entry[t] >= 0, expect), f
    shares = [float((entry[t] >= 0).float().mean()) for t in range(len(atlas.frames))]
    print(f"from frame {mid}: answered share per column {[round(s, 3) for s in shares]}; winners "
          f"{dict(zip(*(a.tolist() for a in np.unique(template.cpu().numpy(), return_counts=True))))}")
    assert all(s > 0 for s in shares[:mid]) and (template[:mid] != mid).all() and (template[mid] == mid).all()
    r, found, tmpl = atlas.best_result_from(mid, 0)
    assert isinstance(r, FlowOUTrackingResult) and torch.equal(found, entry[0] >= 0) and torch.equal(tmpl, template[0])
    assert torch.equal(bits(r.flow), bits(flow[0])) and torch.equal(bits(r.sigma), bits(sigma[0]))
    assert found.any() and torch.isfinite(r.flow[:, found]).all()


# ---- 7. stream ordering ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


@pytest.fixture(scope="module")
def cycles_per_ms():
    return sh.calibrate()


def _best_fixed(ops):
    """Two candidates' inverse planes: template points on the pixel grid pushed about by smooth fields, cells with holes.  Address
    material: the same for every input set."""
    ys, xs = torch.meshgrid(torch.arange(cat.HF, dtype=torch.float32), torch.arange(cat.WF, dtype=torch.float32), indexing="ij")
    tables, cells = [], []
    for k in range(2):
        f, o, s = cat.field(900 + k)
        tables.append(torch.stack([xs + 0.5 * f[0], ys + 0.5 * f[1], o[0] * 0.3, s[0]], -1))
        cells.append(((xs.int() // (7 - 2 * k) + ys.int() // (5 + k)) % 3 - 1).to(torch.int32))
    return {"tables": torch.stack(tables).contiguous().to(DEV), "cells": torch.stack(cells).contiguous().to(DEV)}


def _best_call(ops, fx, inp, v=0):
    from mft_amd import atlas_ops
    slots = np.asarray(cat.FLOW_COLUMNS[v])
    frame_ptrs, lohi_ptrs = ops.trackstore_slot_addresses(*cat._chunks(inp), slots)
    T, HF, WF = slots.shape[1], cat.HF, cat.WF
    return list(atlas_ops.trackstore_flow_from_best(fx["tables"], fx["cells"], [0, 1] if v == 0 else [3, 2], [0, 1] if v == 0 else [1, 0],
                                                    frame_ptrs, lohi_ptrs, torch.full((T, 2, HF, WF), -7.0, device=DEV),
                                                    torch.full((T, 1, HF, WF), -7.0, device=DEV), torch.full((T, 1, HF, WF), -7.0, device=DEV),
                                                    torch.full((T, HF, WF), -7, dtype=torch.int32, device=DEV), columns_per_block=2))


BEST_ENTRY = cat.Entry("trackstore_flow_from_best", ("trackstore_flow_from_best",), _best_fixed, cat._store, _best_call, True, None)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("variants", [(0,), (0, 1)], ids=["one call", "table uploads back to back"])
def test_flow_from_best_runs_on_its_stream(ops, cycles_per_ms, variants):
    run_behind_stall(ops, BEST_ENTRY, cycles_per_ms, variants=variants)


# ---- 8. DenseTrackStore.results_from on a device store -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (9, 34), (37, 53)])
def test_store_results_from_is_its_composition_bitwise(H, W):
    from mft_amd.trackstore import chain_behind_inverse
    frames = {4: const_planes(H, W)}
    frames.update({f: field(f, H, W, 5.0 if f in (7, 9) else 1.5) for f in (7, 5, 9, 1)})
    st = make_store(H, W, frames, device=DEV, frames_per_chunk=2)
    assert len(st._chunks) == 3
    N = H * W
    for src, cols in ((7, None), (9, [1, 4, 9, 9]), (4, [5])):
        got = st.results_from(src, cols)
        table, cell = st.inverse(src)
        tb, found = table.view(N, 4), cell.view(N) >= 0
        q = st.query(torch.where(found[:, None], tb[:, 0:2], torch.zeros((), device=DEV)), cols)
        T = int(q.shape[1])
        want = chain_behind_inverse(tb, q, st._pixel_grid(), found)
        want = (want[0].reshape(T, 2, H, W), want[1].reshape(T, 1, H, W), want[2].reshape(T, 1, H, W))
        assert got[3].dtype == torch.bool and got[3].shape == (H, W) and torch.equal(got[3], found.view(H, W))
        for name, g, w in zip(("flow", "occlusion", "sigma"), got[:3], want):
            assert g.shape == w.shape and g.dtype == torch.float32 and g.is_contiguous(), name
            nan = torch.isnan(w)
            assert torch.equal(torch.isnan(g), nan) and torch.equal(bits(g)[~nan], bits(w.contiguous())[~nan]), name
        lost = ~found.view(H, W)
        if lost.any():
            assert (bits(got[0])[:, :, lost] == NAN_BITS).all() and (bits(got[1])[:, :, lost] == ONE_BITS).all()
            assert (bits(got[2])[:, :, lost] == INF_BITS).all()
    assert st.results_from(7, [])[0].shape == (0, 2, H, W)
