"""tests/chain_reference.py pinned on the CPU: its samplers against ``F.grid_sample`` and its selection against
``Tensor.max(dim=0)``, inf and NaN included; the CPU oracle (oracle/mft_oracle.py) against it in the same value domain; and the
error of the fp32 oracle -- an independent, correct fp32 implementation -- against it, on the inputs of
tests/test_gpu_chain_family.py, as a guard of that file's tolerances from the reference side."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import chain_reference as cr
from oracle import mft_oracle as O

BOUND = 12.0          # units of 2^-24 * S: derived in tests/test_gpu_chain_family.py


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def grid_sample(planes, px, py):
    """torch's sampler, fed the normalised coordinates the reference tracker feeds it."""
    C, H, W = planes.shape
    grid = torch.stack([T(cr.normalised(px, W)), T(cr.normalised(py, H))], -1).reshape(1, 1, -1, 2)
    out = F.grid_sample(T(planes)[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out[0, :, 0].reshape((C,) + np.shape(px)).numpy()


def oracle_sample(planes, px, py):
    W, H = planes.shape[2], planes.shape[1]
    return O.bilinear_zeros(T(planes), O._norm_interp(T(px), W), O._norm_interp(T(py), H)).numpy()


def _points(rng, H, W, n):
    """Fractional points inside, on and around a frame, and the exactly integral ones the round trip keeps integral."""
    px = rng.uniform(-2.5, W + 1.5, n).astype(np.float32)
    py = rng.uniform(-2.5, H + 1.5, n).astype(np.float32)
    px[:8] = [0, 0, W - 1, W - 1, -1, W, 0.5, -0.5]
    py[:8] = [0, H - 1, 0, H - 1, 0, H - 1, -1, H - 0.5]
    return px, py


@pytest.mark.parametrize("H,W", [(2, 2), (5, 5), (6, 8), (37, 53)])
def test_samplers_against_grid_sample_finite(H, W):
    rng = np.random.default_rng([1, H, W])
    planes = (rng.standard_normal((3, H, W)) * 5).astype(np.float32)
    px, py = _points(rng, H, W, 400)
    ref, S = cr.sample_at(planes, px, py)
    for name, got in (("grid_sample", grid_sample(planes, px, py)), ("oracle", oracle_sample(planes, px, py))):
        assert cr.units(got, ref, S) <= BOUND, name
    xy = np.stack([px, py], 1)
    assert np.array_equal(cr.sample_ref(planes, xy)[0], ref)


def _poisoned(H, W, value):
    rng = np.random.default_rng([2, H, W])
    planes = rng.standard_normal((2, H, W)).astype(np.float32)
    planes[0, :, 0] = value
    planes[0, :, -1] = value
    planes[1, 0, :] = value
    planes[1, -1, :] = value
    return planes


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_border_nan_and_inf_do_not_reach_samples_outside(value):
    """Every tap outside the image: 0, whatever the border holds (the issue's 6 x 8 case, which gave 48 NaNs)."""
    H, W = 6, 8
    planes = _poisoned(H, W, value)
    rng = np.random.default_rng(3)
    n = 48
    px = np.concatenate([rng.uniform(-3.0, -1.001, n), rng.uniform(W + 0.001, W + 3, n), rng.uniform(-3, W + 3, 2 * n)]).astype(np.float32)
    py = np.concatenate([rng.uniform(-3, H + 3, 2 * n), rng.uniform(-3.0, -1.001, n), rng.uniform(H + 0.001, H + 3, n)]).astype(np.float32)
    ref, _ = cr.sample_at(planes, px, py)
    assert np.array_equal(ref, np.zeros_like(ref))
    assert np.array_equal(grid_sample(planes, px, py), np.zeros(ref.shape, np.float32))
    assert np.array_equal(oracle_sample(planes, px, py), np.zeros(ref.shape, np.float32))
    # the left operand of the issue's case: every pixel's sample left of the frame
    L = (np.stack([np.full((H, W), -(W + 1.5), np.float32), np.zeros((H, W), np.float32)]), np.zeros((1, H, W), np.float32),
         np.ones((1, H, W), np.float32))
    R = (np.zeros((2, H, W), np.float32), planes[0:1].copy(), planes[0:1].copy())
    got = O.chain(tuple(T(a) for a in L), tuple(T(a) for a in R))
    (rf, ro, rs), _ = cr.chain_ref(L, R)
    assert np.array_equal(got[1].numpy(), ro) and np.array_equal(got[2].numpy(), rs) and not np.isnan(ro).any()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_border_nan_and_inf_with_samples_partly_outside(value):
    """Less than a pixel outside: the border taps inside the image take part (NaN, or +-inf), the others are zeros."""
    H, W = 6, 8
    planes = _poisoned(H, W, value)
    rng = np.random.default_rng(4)
    n = 64
    px = np.concatenate([rng.uniform(-0.9, -0.1, n), rng.uniform(W - 0.9, W - 0.1, n), rng.uniform(1.1, W - 2.1, 2 * n)]).astype(np.float32)
    py = np.concatenate([rng.uniform(1.1, H - 2.1, 2 * n), rng.uniform(-0.9, -0.1, n), rng.uniform(H - 0.9, H - 0.1, n)]).astype(np.float32)
    ref, S = cr.sample_at(planes, px, py)
    assert (~np.isfinite(ref[0, :2 * n])).all() and np.isfinite(ref[0, 2 * n:]).all()
    assert (~np.isfinite(ref[1, 2 * n:])).all() and np.isfinite(ref[1, :2 * n]).all()
    for name, got in (("grid_sample", grid_sample(planes, px, py)), ("oracle", oracle_sample(planes, px, py))):
        assert cr.units(got, ref, S) <= BOUND, name           # (also: NaN and inf exactly where the reference has them)


def test_inf_beside_an_integral_sample_point_is_nan():
    """A tap inside the image takes part even with a zero weight: inf * 0 = NaN (W - 1 and H - 1 powers of two: the
    normalise round trip keeps integral points integral)."""
    H, W = 5, 5
    planes = np.ones((1, H, W), np.float32)
    planes[0, 2, 3] = np.inf
    px = np.array([2, 3, 2, 3, 2.5, 0], np.float32)
    py = np.array([2, 1, 1, 2, 2.0, 0], np.float32)
    ref, S = cr.sample_at(planes, px, py)
    assert np.isnan(ref[0, :3]).all() and np.isposinf(ref[0, 3]) and np.isposinf(ref[0, 4]) and ref[0, 5] == 1.0
    for name, got in (("grid_sample", grid_sample(planes, px, py)), ("oracle", oracle_sample(planes, px, py))):
        assert cr.units(got, ref, S) <= BOUND, name


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------

def torch_select(cands, thr):
    """The reference tracker's selection, restated with torch's own max and gather."""
    flows = torch.stack([T(c[0]) for c in cands])
    occs = torch.stack([T(c[1]) for c in cands])
    sigs = torch.stack([T(c[2]) for c in cands])
    scores = -sigs
    scores[occs > thr] = -float("inf")
    idx = scores.max(dim=0, keepdim=True).indices                      # (1, 1, H, W)
    flow = flows.gather(0, idx.expand(1, 2, *idx.shape[2:]))[0]
    occl = occs.gather(0, idx)[0].clone()
    sigma = sigs.gather(0, idx)[0]
    H, W = flow.shape[1:]
    xs = torch.arange(W, dtype=torch.float32)[None].expand(H, W)
    ys = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    qx, qy = xs + flow[0], ys + flow[1]
    occl[0][(qx < 0) | (qy < 0) | (qx >= W) | (qy >= H)] = 1
    return flow.numpy(), occl.numpy(), sigma.numpy(), idx[0, 0].numpy()


def _chained32(Ls, Rs):
    return [tuple(a.astype(np.float32) for a in cr.chain_ref(L, R)[0]) for L, R in zip(Ls, Rs)]


def _assert_same_selection(cands, thr):
    want = cr.select_ref(cands, thr)
    for name, got in (("torch", torch_select(cands, thr)), ("oracle", [t.numpy() for t in O.select([tuple(T(a) for a in c) for c in cands], thr)])):
        for part, a, b in zip(("flow", "occl", "sigma", "chosen"), got, want):
            assert np.array_equal(cr.bits(a), cr.bits(b)), (name, part)
    return want


@pytest.mark.parametrize("K", [1, 2, 3, 7, 16])
def test_select_ref_against_torch_and_the_oracle(K):
    Ls, Rs = cr.make_case(K, 9, 20, seed=5)
    cands = _chained32(Ls, Rs)
    want = _assert_same_selection(cands, cr.THR)
    if K >= 3:
        sig = np.stack([c[2] for c in cands])
        assert np.isnan(sig).any() and np.isinf(sig).any()                       # NaN scores and infinite sigmas take part,
        assert (np.stack([c[1] for c in cands]) > np.float32(cr.THR)).all(0).any()   # some pixels have every candidate occluded
        assert len(np.unique(want[3])) >= min(K, 3)
    if K >= 2:                                                                   # and exact ties where the tied pair wins
        tie = (cr.bits(cands[0][2]) == cr.bits(cands[1][2])) & (cr.bits(cands[0][1]) == cr.bits(cands[1][1])) & np.isfinite(cands[0][2])
        assert (tie[0] & (want[3] == 0)).any()


def test_selection_corners():
    for name, Ls, Rs, k in cr.selection_corners():
        cands = _chained32(Ls, Rs)
        want = _assert_same_selection(cands, cr.THR)
        assert (want[3] == k).all(), name
    # candidates chained with a right operand of zeros come back bit for bit
    name, Ls, Rs, k = cr.selection_corners()[0]
    for L, c in zip(Ls, _chained32(Ls, Rs)):
        assert all(np.array_equal(cr.bits(a), cr.bits(b)) for a, b in zip(L, c))


# ---------------------------------------------------------------------------
# the fp32 oracle against the reference, on the GPU file's inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", cr.FAMILY_CASES, ids=[c[0] for c in cr.FAMILY_CASES])
@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "inf-nan"])
def test_oracle_chain_within_the_gpu_bound(case, nonfinite):
    """``O.chain`` has the kernel's operation order in float32: a correct implementation meets the bound of
    tests/test_gpu_chain_family.py with room (measured worst case: see that file's docstring), and, with the fixed
    ``bilinear_zeros``, has NaN and inf exactly where the reference has them."""
    _, Ks, H, W, seed = case
    worst = np.zeros(3)
    for Ls, Rs in cr.make_templates(Ks, H, W, seed, nonfinite=nonfinite):
        for L, R in zip(Ls, Rs):
            got = O.chain(tuple(T(a) for a in L), tuple(T(a) for a in R))
            ref, S = cr.chain_ref(L, R)
            worst = np.maximum(worst, [cr.units(g.numpy(), r, s) for g, r, s in zip(got, ref, S)])
    print(f"oracle chain, {case[0]}, {'inf-nan' if nonfinite else 'finite'}: worst error {worst} units of 2^-24 S (flow, occlusion, sigma)")
    assert (worst <= BOUND).all(), worst


def oracle_upsample(flow_lr, ou, mask, P, h, w, pads):
    pl, pr, pt, pb = pads
    outs = []
    for p in range(P):
        sl = slice(p * h * w, (p + 1) * h * w)
        m = T(mask[sl]).reshape(h, w, 576).permute(2, 0, 1)[None]
        f = T(flow_lr[sl]).reshape(h, w, 2).permute(2, 0, 1)[None]
        o = T(ou[sl][:, :3]).reshape(h, w, 3).permute(2, 0, 1)[None]
        crop = lambda t: t[..., pt:8 * h - pb, pl:8 * w - pr]
        flow = crop(O.convex_upsample(f, m, 8.0))
        occl = crop(torch.softmax(O.convex_upsample(o[:, :2], m, 1.0), dim=1)[:, 1:2])
        sigma = crop(torch.sqrt(torch.exp(O.convex_upsample(o[:, 2:3], m, 1.0))))
        outs.append((flow[0], occl[0], sigma[0]))
    return [torch.stack(t).numpy() for t in zip(*outs)]


def test_oracle_upsample_error_figures():
    """The figures behind the upsampler's tolerance in tests/test_gpu_chain_family.py: measured here, on exactly that file's
    inputs, and asserted not to exceed what chain_reference.UP_ORACLE_UNITS records."""
    worst = dict(flow=0.0, occl=0.0, sigma=0.0)
    for P in (1, 3):
        for h, w in cr.UP_SHAPES:
            for pads in cr.UP_PADS:
                flow_lr, ou, mask = cr.upsample_inputs(P, h, w, 4, seed=7)
                ref, N = cr.upsample_ref(flow_lr, ou, mask, P, h, w, pads)
                u = cr.upsample_units(oracle_upsample(flow_lr, ou, mask, P, h, w, pads), ref, N)
                worst = {k: max(worst[k], u[k]) for k in worst}
    print("fp32 oracle against upsample_ref, worst error in units of 2^-24 max(1, largest neighbour):", worst)
    for k in worst:
        assert worst[k] <= cr.UP_ORACLE_UNITS[k], (k, worst[k])
        assert worst[k] >= cr.UP_ORACLE_UNITS[k] / 2, (k, worst[k])      # the recorded figure is the measured one, not a loose cap


def test_upsample_ref_basics():
    """A one-hot mask copies one neighbour (zeros outside); the crop is the crop of the full result; ``ld`` does not matter."""
    P, h, w = 2, 3, 4
    flow_lr, ou, mask = cr.upsample_inputs(P, h, w, 7, seed=8)
    mask[:] = -1e4
    mask.reshape(P, h, w, 9, 64)[:, :, :, 5, :] = 0                     # k = 5: neighbour (y, x + 1)
    (flow, occl, sigma), _ = cr.upsample_ref(flow_lr, ou, mask, P, h, w)
    f = flow_lr.reshape(P, h, w, 2).astype(np.float64)
    assert np.allclose(flow[1, 0, 8:16, 0:8], 8 * f[1, 1, 1, 0], rtol=1e-12) and np.all(flow[:, :, :, -8:] == 0)
    assert np.allclose(sigma[0, 0, 0:8, 8:16], np.exp(np.float64(ou[2, 2]) / 2), rtol=1e-12)
    (f2, o2, s2), _ = cr.upsample_ref(flow_lr, ou[:, :3], mask, P, h, w, (3, 4, 1, 2))
    assert np.array_equal(f2, flow[..., 1:-2, 3:-4]) and np.array_equal(o2, occl[..., 1:-2, 3:-4]) and np.array_equal(s2, sigma[..., 1:-2, 3:-4])
