"""tests/corr_reference.py against torch and the oracle on the CPU: the references the GPU tests of the correlation family
(tests/test_gpu_corr_family.py) trust must themselves be pinned, and the inputs they call exact must be exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_reference as cr
from oracle import mft_oracle as O

# grid_sample and the oracle normalise by (size - 1): levels of width or height 1 are left to the exact GPU tests
NORMALISABLE = [(P, h, w) for P, h, w in cr.SHAPES if (h >> 3) >= 2 and (w >> 3) >= 2]


def _gauss_levels(N, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((N, h >> l, w >> l)).astype(np.float32) for l in range(4)]


def _gauss_case(P, h, w, seed=5, quantum=None):
    """Gaussian levels; the edge coordinates (on and beyond every edge of every level) and the same with a Gaussian perturbation
    that takes them off the quarter grid (rounded to multiples of `quantum` if given)."""
    N = P * h * w
    rng = np.random.default_rng(seed + 1)
    edge = cr.edge_coords(P, h, w)[0]
    off = edge.astype(np.float64) + rng.standard_normal(edge.shape) * 0.37
    if quantum:
        off = np.round(off / quantum) * quantum
    return _gauss_levels(N, h, w, seed), [edge, off.astype(np.float32)]


@pytest.mark.parametrize("P,h,w", NORMALISABLE)
def test_lookup_ref_vs_grid_sample_fp64(P, h, w):
    """F.grid_sample in float64 (align_corners=True, zeros) at s + (a - 4), s the float32 level coordinate: its normalise round
    trip moves a coordinate by a few 2^-52 of its size, nothing else differs -- 1e-9 max|tap|.  "Nothing else" needs the float32
    steps of the definition (s - floor(s), 1 - f, the weight products) to be exact, or float64 weights differ from them by 2^-24:
    the Gaussian coordinates are multiples of 2^-8, so f is a multiple of 2^-11 at level 3 and a product one of 2^-22.  (What the
    float32 steps do to arbitrary coordinates is part of the definition; test_fp32_blend_within_the_derived_bound and the GPU
    test on real-valued inputs evaluate them.)"""
    levels, coord_sets = _gauss_case(P, h, w, quantum=2.0 ** -8)
    N = P * h * w
    d = torch.arange(-4, 5, dtype=torch.float64)
    for coords in coord_sets:
        got, _ = cr.lookup_ref(levels, coords)
        got = got.reshape(N, 4, 9, 9)
        for l, level in enumerate(levels):
            hl, wl = level.shape[1:]
            s = torch.from_numpy(coords / np.float32(1 << l)).double()
            px = s[:, 0, None, None] + d[None, :, None] + 0 * d[None, None, :]         # [n, a, b]
            py = s[:, 1, None, None] + d[None, None, :] + 0 * d[None, :, None]
            grid = torch.stack([2 * px / (wl - 1) - 1, 2 * py / (hl - 1) - 1], -1)
            want = F.grid_sample(torch.from_numpy(level).double()[:, None], grid, mode="bilinear", padding_mode="zeros",
                                 align_corners=True)[:, 0].numpy()
            assert np.abs(got[:, l] - want).max() <= 1e-9 * np.abs(level).max(), l


@pytest.mark.parametrize("P,h,w", [(1, 17, 23), (1, 16, 24)])
def test_lookup_ref_vs_oracle(P, h, w):
    """oracle.mft_oracle.corr_lookup (fp32, through the normalise round trip) at the bound the suite uses for it: pins the
    channel order l * 81 + a * 9 + b and the level order."""
    levels, coord_sets = _gauss_case(P, h, w, seed=9)
    N = h * w
    pyr = [torch.from_numpy(t).reshape(N, 1, h >> l, w >> l) for l, t in enumerate(levels)]
    for coords in coord_sets:
        want = O.corr_lookup(pyr, torch.from_numpy(coords.T.reshape(1, 2, h, w).copy()))
        got, _ = cr.lookup_ref(levels, coords)
        assert np.abs(got - want[0].reshape(324, N).T.double().numpy()).max() < 1e-4


@pytest.mark.parametrize("h,w", [(9, 15), (17, 23), (8, 8)])
def test_pyramid_refs_vs_oracle_and_avg_pool(h, w):
    rng = np.random.default_rng(h)
    f1 = rng.standard_normal((1, h, w, 32)).astype(np.float32)
    f2 = rng.standard_normal((1, h, w, 32)).astype(np.float32)
    t1, t2 = (torch.from_numpy(f).permute(0, 3, 1, 2).contiguous() for f in (f1, f2))
    want = O.corr_pyramid(O.corr_volume(t1, t2))
    for l, got in enumerate(cr.pyramid_ref(f1, f2)):
        assert got.shape == (h * w, h >> l, w >> l)
        assert np.abs(got - want[l][:, 0].double().numpy()).max() < 2e-5, l
    ref = t2.double()
    for l, got in enumerate(cr.feature_pyramid_ref(f2)):
        assert np.array_equal(got, ref.permute(0, 2, 3, 1).numpy()), l
        ref = F.avg_pool2d(ref, 2, stride=2) if min(ref.shape[-2:]) >= 2 else ref


@pytest.mark.parametrize("P,h,w", cr.SHAPES)
def test_shared_inputs_are_exact(P, h, w):
    """The exactness conditions of every shared input (each builder asserts its own), and what the coordinate builder promises."""
    case = cr.exact_case(P, h, w)
    N = P * h * w
    coords = case["coords"].reshape(-1, 2)
    assert case["coords"].shape[1] == N and np.array_equal(coords * 4, np.round(coords * 4))
    assert float(np.abs(case["want"]).max()) <= 448.0 and float(np.abs(case["want"]).max()) > 300.0
    assert np.array_equal(case["want"] * 1024, np.round(case["want"] * 1024))
    have = {(float(x), float(y)) for x, y in coords}
    for l in range(4):
        sc, wl, hl = float(1 << l), w >> l, h >> l
        for x in (-5.25 * sc, -4.75 * sc, (wl + 4) * sc, (wl + 3.75) * sc):
            assert any(p[0] == x and 0 <= p[1] < h for p in have), (l, x)
            for y in (-5.25 * sc, -4.75 * sc, (hl + 4) * sc, (hl + 3.75) * sc):
                assert (x, y) in have
        for y in (-5.25 * sc, -4.75 * sc, (hl + 4) * sc, (hl + 3.75) * sc):
            assert any(p[1] == y and 0 <= p[0] < w for p in have), (l, y)
        # what these points are for: the window wholly outside / exactly one column inside, on either side
        x0 = cr.lookup_weights(np.array([[-5.25 * sc, 0], [-4.75 * sc, 0], [(wl + 4) * sc, 0], [(wl + 3.75) * sc, 0]], np.float32), l)[0]
        inside = [int(((x0[i] + np.arange(10) >= 0) & (x0[i] + np.arange(10) < wl)).sum()) for i in range(4)]
        assert inside == [0, 1, 0, 1], (l, inside)
    for y in range(h):
        for x in range(w):
            assert (float(x), float(y)) in have
    assert coords[:, 0].min() <= -40 and coords[:, 0].max() >= w + 40 and coords[:, 1].min() <= -40 and coords[:, 1].max() >= h + 40
    f1, f2 = cr.exact_features(P, h, w)
    assert f1.shape == (P, h, w, 256) and np.count_nonzero(f1) == N and float(np.abs(f2).max()) == 448.0
    # the on-device construction of the large case gives the same taps
    n = torch.arange(N, dtype=torch.int64)[:, None, None]
    for l in range(4):
        t = cr.level_values(n, l, torch.arange(h >> l)[None, :, None], torch.arange(w >> l)[None, None, :])
        assert np.array_equal(t.numpy().astype(np.float32), case["levels"][l]), l


def test_hostile_cells_in_the_reference():
    """Non-finite coordinates give NaN in all 324 channels, huge finite ones 0 -- and the neighbours are untouched."""
    P, h, w = 1, 8, 8
    case = cr.exact_case(P, h, w)
    base = case["coords"][1]
    hostile, nan_rows, zero_rows = cr.hostile_coords(base)
    assert len(nan_rows) == 6 and len(zero_rows) == 20 and len(set(nan_rows) | set(zero_rows)) == 26
    got, _ = cr.lookup_ref(case["levels"], hostile)
    assert np.isnan(got[nan_rows]).all() and (got[zero_rows] == 0).all()
    rest = np.setdiff1d(np.arange(P * h * w), np.concatenate([nan_rows, zero_rows]))
    assert np.array_equal(got[rest], case["want"][1][rest])


def test_fp32_blend_within_the_derived_bound():
    """A plain float32 evaluation of the blend stays within 8 * 2^-24 * mag of lookup_ref on Gaussian inputs.  The bound allows a
    kernel three roundings per weight (1 - fx, 1 - fy, their product), four products and three sums, and one unit to spare; this
    evaluation shares the reference's weights, so it can use the products' and sums' four units at most.
    Worst share observed: 0.357 of the bound (2.9 units)."""
    worst = 0.0
    for P, h, w in [(1, 17, 23), (2, 9, 15), (1, 12, 33)]:
        levels, coord_sets = _gauss_case(P, h, w, seed=21)
        for coords in coord_sets:
            want, mag = cr.lookup_ref(levels, coords)
            err = np.abs(cr.lookup_f32(levels, coords).astype(np.float64) - want)
            assert (err <= cr.LOOKUP_BOUND_UNITS * cr.EPS * mag).all()
            worst = max(worst, float((err / np.maximum(cr.LOOKUP_BOUND_UNITS * cr.EPS * mag, 1e-300)).max()))
    print(f"fp32 blend: worst share of the 8 EPS mag bound {worst:.3f}")
    assert worst > 0.02          # (the check is not vacuous: rounding errors do occur)
