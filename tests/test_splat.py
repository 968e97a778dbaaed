"""The integer forward splat and the overlay arithmetic of csrc/splat.hip, restated in numpy (int64, fp32 weights, ``np.rint``,
``np.add.at``) and checked on the CPU: against the reference's own ``warp_forward`` outputs (tests/golden/results_api.npz),
against the host overlay path (``vis.draw_edit``), and the fixed-point plan (``ops.splat_plan``).  The GPU tests
(tests/test_gpu_splat.py) compare the kernels with these restatements bit for bit."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from mft_amd import ops, vis
from mft_amd.results import FlowOUTrackingResult

F32 = np.float32


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------

def splat_corners(flow, keep, S):
    """flow [2,H,W] fp32, keep [H,W] bool -> (kept [H,W] bool, 4 x destination index, 4 x quantised weight), corners in the
    order (y0,x0), (y1,x0), (y0,x1), (y1,x1); kept source pixels in row-major order."""
    _, H, W = flow.shape
    gy, gx = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        x = gx.astype(F32) + flow[0].astype(F32)
        y = gy.astype(F32) + flow[1].astype(F32)
    keep = keep & np.isfinite(x) & np.isfinite(y)
    x, y = x[keep], y[keep]
    x0 = np.clip(np.floor(x), F32(-1.0e6), F32(1.0e6)).astype(np.int64)
    y0 = np.clip(np.floor(y), F32(-1.0e6), F32(1.0e6)).astype(np.int64)
    xc, yc = np.clip(x, F32(0), F32(W - 1)), np.clip(y, F32(0), F32(H - 1))
    x0c, x1c = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    y0c, y1c = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    wx0, wx1 = x1c.astype(F32) - xc, xc - x0c.astype(F32)
    wy0, wy1 = y1c.astype(F32) - yc, yc - y0c.astype(F32)
    w = [wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1]
    assert all(a.dtype == F32 for a in w)
    p = [y0c * W + x0c, y1c * W + x0c, y0c * W + x1c, y1c * W + x1c]
    q = [np.rint(a.astype(np.float64) * 2.0 ** S).astype(np.int64) for a in w]
    return keep, p, q


def splat_accumulate(flow, vq, keep, S):
    """vq [H,W,C] int64 -> accumulator [C+1, H*W] int64 (row C: the weight sums)."""
    _, H, W = flow.shape
    C = vq.shape[2]
    keep, p, q = splat_corners(flow, keep, S)
    v = vq[keep]                                            # [n, C]
    acc = np.zeros((C + 1, H * W), np.int64)
    for pj, qj in zip(p, q):
        nz = qj != 0                                        # a corner with q_w == 0 is dropped
        for c in range(C):
            np.add.at(acc[c], pj[nz], v[nz, c] * qj[nz])
        np.add.at(acc[C], pj[nz], qj[nz])
    return acc


def splat_forward(flow, img, mask=None, border=None, bound=None):
    """The restated ``warp_forward_device``: img [H,W,C] float32 or uint8 -> (float32 [H,W,C], hit [H,W] bool, plan)."""
    H, W, C = img.shape
    if img.dtype == np.uint8:
        plan = ops.splat_plan(H, W, 8, False)
        vq = img.astype(np.int64)
    else:
        bound = float(np.abs(img).max()) if bound is None else bound
        plan = ops.splat_plan(H, W, ops.value_bits(bound), True)
        vq = np.rint(img.astype(np.float64) * 2.0 ** plan.V).astype(np.int64)
    assert plan.native
    keep = np.ones((H, W), bool) if mask is None else np.asarray(mask).astype(bool)
    acc = splat_accumulate(flow, vq, keep, plan.S)
    cnt = acc[C]
    hit = cnt > 0
    out = np.full((H * W, C), 0.0 if border is None else border, F32)
    den = cnt[hit].astype(np.float64) * 2.0 ** plan.V
    out[hit] = (acc[:C, hit].astype(np.float64) / den).astype(F32).T
    return out.reshape(H, W, C), hit.reshape(H, W), plan


def overlay_edit(flow, occl, edit, frame):
    """The restated ``mftx_overlay_edit``: edit [H,W,4] uint8 BGRA, frame [H,W,3] uint8 -> [H,W,3] uint8."""
    H, W = frame.shape[:2]
    plan = ops.splat_plan(H, W, 16, False)
    assert plan.native and plan.V == 0
    with np.errstate(invalid="ignore"):
        keep = (occl.reshape(H, W) < F32(0.5)) & (edit[..., 3] > 0)
    a = edit[..., 3].astype(np.int64)
    vq = np.stack([edit[..., 0].astype(np.int64) * a, edit[..., 1].astype(np.int64) * a, edit[..., 2].astype(np.int64) * a, a], -1)
    acc = splat_accumulate(flow, vq, keep, plan.S)
    cnt = acc[4]
    hit = cnt > 0
    dc = cnt[hit].astype(np.float64)
    colour = np.zeros((H * W, 3), F32)
    colour[hit] = (acc[:3, hit].astype(np.float64) / (dc * 255.0)).astype(F32).T
    colour = np.clip(colour, 0, 255).astype(np.uint8)
    alpha = np.zeros(H * W, F32)
    alpha[hit] = (acc[3, hit].astype(np.float64) / dc).astype(F32) / F32(ops.edit_alpha_divisor(edit))
    f = frame.reshape(H * W, 3).astype(np.int64)
    gray = ((f[:, 0] * 1868 + f[:, 1] * 9617 + f[:, 2] * 4899 + (1 << 13)) >> 14).astype(F32)
    out = colour.astype(F32) + gray[:, None] * (F32(1) - alpha)[:, None]
    assert out.dtype == F32
    return np.clip(out, 0, 255).astype(np.uint8).reshape(H, W, 3)


def overlay_case(H, W, seed):
    """Seeded overlay inputs: a smooth flow that leaves the frame, a smooth occlusion field crossing 0.5, a random uint8 BGRA
    edit with a quarter of its alpha set to 0, a random frame."""
    r = gi._rng(97, seed)
    flow = gi.smooth_field(r, 2, H, W, cells=3, amp=5.0)
    flow[:, :, : W // 8] -= 7.0                              # the left columns leave the frame
    occl = np.clip(0.5 + gi.smooth_field(r, 1, H, W, cells=4, amp=0.4), 0, 1).astype(F32)
    edit = r.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    edit[..., 3][r.random((H, W)) < 0.25] = 0
    frame = r.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return dict(flow=flow.astype(F32), occl=occl, edit=edit, frame=frame)


OVERLAY_CASES = [(40, 56, 0), (61, 67, 1)]


def within_one_level(got, want, cap=0.005):
    """The host path truncates floats to uint8: a value within ~1e-4 of an integer may land one level off.  Two conditions:
    every channel value within 1 level, at most 0.5 % of the values different at all."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return int(d.max()), float((d != 0).mean()), bool(d.max() <= 1 and (d != 0).mean() <= cap)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "results_api.npz")


def test_restatement_matches_reference_golden(g):
    d = gi.results_api_inputs()
    res = FlowOUTrackingResult(torch.from_numpy(d["flow"]), torch.from_numpy(d["occl"]), torch.from_numpy(d["sigma"]))
    for mask, border, key in ((None, None, "warp_forward"), (d["mask"], -1.0, "warp_forward_masked")):
        out, hit, plan = splat_forward(d["flow"], d["img"], mask=mask, border=border)
        assert (plan.S, plan.V) == (24, 23)
        diff = np.abs(out - g[key]).max()
        print(f"{key}: max |restatement - reference| = {diff:.3g}, {int(hit.sum())} hit pixels")
        assert np.allclose(out, g[key], atol=1e-5)
        # the hit set: the torch path marks pixels nothing reached with the border value
        want_hit = (res.warp_forward(np.ones((40, 56, 1), F32), mask=mask, border=-1.0)[..., 0] != -1.0)
        assert np.array_equal(hit, want_hit)
        if border is not None:
            assert np.array_equal(hit, (g[key] != -1.0).all(-1))


def test_splat_plan_bounds_and_refusals():
    sizes = [(1, 1), (1, 2), (3, 5), (40, 56), (61, 67), (128, 160), (512, 512), (1080, 1920), (2160, 3840), (4320, 7680)]
    sizes += [(1 << a, 1 << b) for a in range(0, 13) for b in range(0, 13) if (1 << (a + b)) <= 4320 * 7680]
    sizes += [((1 << a) + 1, 1) for a in range(0, 25)]            # just past every power of two
    for H, W in sizes:
        L = ops.splat_plan(H, W, 0, False).L
        assert 2 ** L >= 4 * H * W and (L == 0 or 2 ** (L - 1) < 4 * H * W)
        for k in range(17):
            for floating in (False, True):
                p = ops.splat_plan(H, W, k, floating)
                assert p.L + k + p.V + p.S <= 62 and p.S <= 24 and p.V <= 23
                assert p.native == (p.V >= 12 if floating else p.S >= 16)
                if floating:
                    assert p.S == 24 and p.V == min(23, 62 - p.L - k - 24)
                else:
                    assert p.V == 0 and p.S == min(24, 62 - p.L - k)
    assert ops.splat_plan(40, 56, 0, True)[:2] == (24, 23)
    assert ops.splat_plan(512, 512, 16, False)[:2] == (24, 0)
    p = ops.splat_plan(4320, 7680, 16, False)                   # the edit overlay at 8K: L = 27, 19 weight bits, still native
    assert (p.L, p.S, p.native) == (27, 19, True)
    assert not ops.splat_plan(4320, 7680, 16, True).native       # float values below 2^16 at 8K: V = -5
    assert not ops.splat_plan(4320, 7680, 0, True).native        # V = 11
    assert ops.splat_plan(2160, 3840, 1, True) == (24, 12, 25, True)
    assert not ops.splat_plan(1 << 12, 1 << 12, 21, False).native   # S = 15
    assert [ops.value_bits(b) for b in (0.0, 0.5, 0.999, 1.0, 1.5, 2.0, 255.0, 256.0, 65025.0)] == [0, 0, 0, 1, 1, 2, 8, 9, 16]


@pytest.mark.parametrize("H,W,seed", OVERLAY_CASES)
def test_overlay_restatement_matches_host_path(H, W, seed):
    c = overlay_case(H, W, seed)
    occ = c["occl"]
    assert (occ < 0.5).any() and (occ > 0.5).any() and (c["edit"][..., 3] == 0).mean() > 0.15
    res = FlowOUTrackingResult(torch.from_numpy(c["flow"]), torch.from_numpy(occ), torch.zeros(1, H, W))
    assert res.invalid_mask().any()                              # the flow leaves the frame
    want = vis.draw_edit(c["frame"], res, c["edit"])
    got = overlay_edit(c["flow"], occ, c["edit"], c["frame"])
    worst, frac, ok = within_one_level(got, want)
    print(f"{H} x {W}: max {worst} level(s), {100 * frac:.4f} % of the values differ")
    assert ok, (worst, frac)
    assert (got != vis.to_gray_3ch(c["frame"])).any(-1).mean() > 0.1     # the edit covers a good part of the frame


def test_library_exports_splat_symbols():
    from mft_amd import _lib
    names = ("mftx_splat_forward", "mftx_splat_resolve", "mftx_overlay_edit", "mftx_overlay_dots")
    assert all(n in _lib.SIGNATURES for n in names)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.mftx_version() == 400
