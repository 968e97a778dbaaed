"""Exact references, in plain numpy, for the kernels of csrc/chain.hip and csrc/upsample.hip -- TEST INFRASTRUCTURE.

What the kernels and these references share is the DEFINITION of the operation, not its arithmetic:

* The sampling coordinates are part of the definition (the reference tracker computes them in float32, and a sample point that
  lands on the other side of a pixel centre reads other taps), so they are computed here in numpy float32, operation by
  operation as the kernels do: ``px = x + flow_x``, ``ix = ((px * float32(2 / (W - 1)) - 1) + 1) / 2 * (W - 1)``,
  ``x0 = floor(ix)``, ``wx = ix - x0`` (numpy never contracts a product and a sum into an FMA).
* Everything after that is float64: the four weights, the four taps, the sums, the square root.
* A tap outside the image is 0 whatever lies at a clamped address (``np.where(inside, tap, 0)``): that is what
  ``F.grid_sample(padding_mode='zeros')`` does on the CPU, which never reads such a tap.  A tap INSIDE the image takes part with
  its weight even when the weight is zero, so ``inf * 0 = NaN`` there -- also what grid_sample does.
* The selection is the reference's rule, literally: ``scores = where(occl > thr, -inf, -sigma)``, ``k = argmax(scores)`` --
  numpy's argmax returns the first NaN if there is one, else the first maximum, exactly like ``Tensor.max(dim=0).indices``.

Every sampler also returns the per-pixel scale S a tolerance is expressed in (see tests/test_gpu_chain_family.py for the bound):
the sum of the magnitudes that enter a flow component, the largest magnitude that enters an occlusion or a sigma.

tests/test_chain_reference.py pins this module against torch on the CPU (finite inputs, inf and NaN)."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24           # half an ulp of 1.0f: the relative rounding error of one fp32 operation


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=F32)


def unnormalised(p, size):
    """Pixel coordinate -> normalised -> pixel coordinate, in float32 (csrc/grid_sample.h, ``grid_sample_at``)."""
    p = _f32(p)
    s = F32(2 / (size - 1))
    return ((p * s - F32(1)) + F32(1)) / F32(2) * F32(size - 1)


def normalised(p, size):
    """The normalised coordinate ``F.grid_sample`` is handed: ``p * float32(2 / (size - 1)) - 1`` in float32."""
    return _f32(p) * F32(2 / (size - 1)) - F32(1)


def sample_at(planes, px, py):
    """planes (C, H, W) float32; px, py float32 arrays of one shape: pixel coordinates before the normalise round trip.
    -> (samples float64 (C, ...), largest |tap| inside the image float64 (C, ...))."""
    planes = _f32(planes)
    C, H, W = planes.shape
    ix, iy = unnormalised(px, W), unnormalised(py, H)
    assert ix.dtype == F32 and iy.dtype == F32
    fx, fy = np.floor(ix), np.floor(iy)
    wx, wy = (ix - fx).astype(np.float64), (iy - fy).astype(np.float64)       # the subtraction is float32: part of the definition
    x0 = np.clip(fx, F32(-1.0e6), F32(1.0e6)).astype(np.int64)                 # (beyond any image: every tap outside)
    y0 = np.clip(fy, F32(-1.0e6), F32(1.0e6)).astype(np.int64)
    out = np.zeros((C,) + ix.shape, np.float64)
    big = np.zeros((C,) + ix.shape, np.float64)
    pl = planes.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy, vy in ((0, 1.0 - wy), (1, wy)):
            for dx, vx in ((0, 1.0 - wx), (1, wx)):
                xx, yy = x0 + dx, y0 + dy
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                tap = np.where(inside[None], pl[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0)
                out = out + tap * (vx * vy)[None]
                big = np.maximum(big, np.abs(tap))
    return out, big


def sample_ref(planes, xy):
    """The sampler at given points: planes (C, H, W), xy (N, 2) float32 -> (samples (C, N), largest |tap| (C, N)), float64."""
    xy = _f32(xy)
    return sample_at(planes, xy[:, 0], xy[:, 1])


def _grid(H, W):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return xs.astype(F32), ys.astype(F32)


def chain_ref(L, R):
    """L, R = (flow (2, H, W), occl (1, H, W), sigma (1, H, W)) float32 -> ((flow, occl, sigma) float64, (S_flow, S_occl, S_sigma))."""
    flowL, occL, sigL = (_f32(a) for a in L)
    flowR, occR, sigR = (_f32(a) for a in R)
    _, H, W = flowL.shape
    gx, gy = _grid(H, W)
    px, py = gx + flowL[0], gy + flowL[1]                              # float32
    assert px.dtype == F32
    sf, bf = sample_at(flowR, px, py)
    so, bo = sample_at(occR, px, py)
    ss, bs = sample_at(sigR, px, py)
    p64 = np.stack([px, py]).astype(np.float64)
    g64 = np.stack([gx, gy]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        flow = (p64 + sf) - g64
        occl = np.maximum(occL.astype(np.float64), so)                 # np.maximum propagates a NaN of either side
        sigma = np.sqrt(sigL.astype(np.float64) ** 2 + ss ** 2)
        S = (np.abs(p64) + np.abs(g64) + bf, np.maximum(np.abs(occL.astype(np.float64)), bo),
             np.maximum(np.abs(sigL.astype(np.float64)), bs))
    return (flow, occl, sigma), S


def select_ref(cands, thr):
    """cands: K x (flow (2, H, W), occl (1, H, W), sigma (1, H, W)) float32 -> flow, occl, sigma (float32, copies of the chosen
    candidate's values) and the chosen index (H, W) int64."""
    flows = np.stack([_f32(c[0]) for c in cands])
    occs = np.stack([_f32(c[1]) for c in cands])
    sigs = np.stack([_f32(c[2]) for c in cands])
    _, _, H, W = flows.shape
    with np.errstate(invalid="ignore"):
        scores = np.where(occs > F32(thr), F32(-np.inf), -sigs)        # (a NaN occlusion is not > thr: not suppressed)
    k = np.argmax(scores, axis=0)                                      # (1, H, W): first NaN, else first maximum
    flow = np.take_along_axis(flows, np.broadcast_to(k[None], (1, 2, H, W)), 0)[0]
    occl = np.take_along_axis(occs, k[None], 0)[0].copy()
    sigma = np.take_along_axis(sigs, k[None], 0)[0]
    gx, gy = _grid(H, W)
    qx, qy = gx + flow[0], gy + flow[1]                                # float32
    assert qx.dtype == F32
    occl[0][(qx < 0) | (qy < 0) | (qx >= F32(W)) | (qy >= F32(H))] = 1
    return flow, occl, sigma, k[0]


def upsample_ref(flow_lr, ou, mask, P, h, w, pads=(0, 0, 0, 0)):
    """Convex 8x upsampling with the flow wrapper's post-processing, in float64.  flow_lr (P h w, 2), ou (P h w, ld >= 3: two
    occlusion logits, log-variance; further columns are never read), mask (P h w, 576: channel k * 64 + sy * 8 + sx, k = ky * 3 + kx).
    -> (flow (P, 2, H0, W0), occl (P, 1, H0, W0), sigma (P, 1, H0, W0)), and per output pixel the largest magnitude among the
    nine neighbours it blends: (N_flow (P, 2, H0, W0) of the x8 flow, N_logit (P, 1, ..) of both logits, N_u (P, 1, ..))."""
    pl, pr, pt, pb = pads
    x = np.concatenate([np.asarray(flow_lr, np.float64).reshape(P, h, w, 2) * 8.0,
                        np.asarray(ou, np.float64).reshape(P, h, w, -1)[..., :3]], -1)       # (P, h, w, 5)
    m = np.asarray(mask, np.float64).reshape(P, h, w, 9, 8, 8)
    m = np.exp(m - m.max(3, keepdims=True))
    m = m / m.sum(3, keepdims=True)
    xp = np.zeros((P, h + 2, w + 2, 5))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((P, h, w, 8, 8, 5))
    big = np.zeros((P, h, w, 5))
    for k in range(9):
        ky, kx = divmod(k, 3)
        nb = xp[:, ky:ky + h, kx:kx + w]                                # x[y + ky - 1, x + kx - 1], zeros outside
        out += m[:, :, :, k, :, :, None] * nb[:, :, :, None, None, :]
        big = np.maximum(big, np.abs(nb))
    out = out.transpose(0, 5, 1, 3, 2, 4).reshape(P, 5, 8 * h, 8 * w)
    big = np.broadcast_to(big[:, :, :, None, None, :], (P, h, w, 8, 8, 5)).transpose(0, 5, 1, 3, 2, 4).reshape(P, 5, 8 * h, 8 * w)
    out, big = (a[:, :, pt:8 * h - pb, pl:8 * w - pr] for a in (out, big))
    l0, l1, u = out[:, 2:3], out[:, 3:4], out[:, 4:5]
    lm = np.maximum(l0, l1)
    e0, e1 = np.exp(l0 - lm), np.exp(l1 - lm)
    return (out[:, 0:2], e1 / (e0 + e1), np.exp(u / 2)), (big[:, 0:2], np.maximum(big[:, 2:3], big[:, 3:4]), big[:, 4:5])


# ---------------------------------------------------------------------------
# seeded inputs, shared by tests/test_chain_reference.py (CPU) and tests/test_gpu_chain_family.py
# ---------------------------------------------------------------------------

THR = 0.02
SPREADS = (0.3, 3.0, 40.0)         # left flows: sub-pixel, a few pixels, mostly out of a small frame
SIZES = ((2, 2), (5, 4), (3, 259), (2, 260), (37, 53))
KS = (1, 4, 5, 8, 9, 16)


def make_result(rng, H, W, spread, left, nonfinite, occluded=False):
    """One (flow, occl, sigma) triple.  Flows are finite.  Occlusions lie on both sides of and exactly at the threshold; sigmas
    are positive and at most 1e6 (so that float32 squares stay finite where float64's do).  A left operand also holds flows
    beyond the kernels' +-1e6 clamp and beyond the int range, and flows that leave the frame by less and by more than a pixel on
    its border pixels; a right operand holds, with ``nonfinite``, +inf and NaN on its border rows and columns; both hold them at
    a few pixels anywhere."""
    flow = (rng.standard_normal((2, H, W)) * spread).astype(F32)
    occl = (rng.random((1, H, W)) * 0.05).astype(F32)
    if occluded:
        occl += F32(0.5)
    sigma = (rng.random((1, H, W)) + 0.1).astype(F32)
    pick = rng.random((1, H, W))
    occl[pick < 0.06] = F32(THR)                                       # exactly at the threshold: not occluded
    occl[pick < 0.03] = np.nextafter(F32(THR), F32(1))                 # the next float above it: occluded
    border = np.zeros((H, W), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    if left:
        pick = rng.random((H, W))
        for lo, v in ((0.00, 3e9), (0.01, -3e9), (0.02, 1e30), (0.03, -1e30)):
            m = (pick >= lo) & (pick < lo + 0.01)
            flow[rng.integers(0, 2)][m] = F32(v)
        # leave the frame through the nearest edge by 0.5 px (less than a pixel) or by 1.7 px (more), on half of the border pixels
        ys, xs = np.nonzero(border & (rng.random((H, W)) < 0.5))
        for y, x in zip(ys, xs):
            by = F32(0.5) if rng.random() < 0.5 else F32(1.7)
            if x == 0:
                flow[0, y, x] = -by
            elif x == W - 1:
                flow[0, y, x] = by
            if y == 0:
                flow[1, y, x] = -by
            elif y == H - 1:
                flow[1, y, x] = by
        flow[:, 0, 0] = 0                                              # an exactly integral sample point: zero weights on taps inside
        pick = rng.random((1, H, W))
        sigma[pick < 0.04] = F32(1e6)                                  # sqrt(1e12 + s^2) = 1e6 in float32 for s < 100: exact ties
    where = rng.random((1, H, W))                                     # (drawn whether used or not: the finite case keeps its values)
    edge = np.where(border[None], rng.random((1, H, W)), 1.0)
    if nonfinite:
        lim = 0.02 if left else 0.01
        occl[where < lim] = np.nan
        occl[(where >= lim) & (where < 2 * lim)] = np.inf
        sigma[(where >= 2 * lim) & (where < 3 * lim)] = np.nan
        sigma[(where >= 3 * lim) & (where < 4 * lim)] = np.inf
        if not left:
            occl[edge < 0.06] = np.nan
            occl[(edge >= 0.06) & (edge < 0.12)] = np.inf
            sigma[(edge >= 0.12) & (edge < 0.18)] = np.nan
            sigma[(edge >= 0.18) & (edge < 0.24)] = np.inf
    return flow, occl, sigma


def make_case(K, H, W, seed, nonfinite=True):
    """K (left, right) pairs, numpy float32: -> (Ls, Rs).  The same seed without ``nonfinite`` gives the same values except for
    the inf and NaN entries (the generator draws the same numbers either way)."""
    rng = np.random.default_rng([seed, K, H, W])
    Ls = [make_result(rng, H, W, SPREADS[(k + seed) % 3], True, nonfinite) for k in range(K)]
    Rs = [make_result(rng, H, W, 3.0, False, nonfinite) for k in range(K)]
    if K >= 3:                                                         # a stretch of pixels where every candidate is occluded
        n = max(1, (H * W) // 16)
        for L in Ls:
            L[1].reshape(-1)[-n:] = F32(0.7)
    if K >= 2:                                                         # exact ties between candidates 0 and 1 wherever they win
        Rs[1] = Rs[0]
        _tie(rng, Ls, 0, 1)
    return Ls, Rs


def _tie(rng, Ls, a, b):
    """Left operand b takes a's values on a third of the pixels: with one right operand for both, the two chained candidates are
    equal bit for bit there."""
    m = rng.random(Ls[a][1].shape[1:]) < 0.33
    for pa, pb in zip(Ls[a], Ls[b]):
        pb[:, m] = pa[:, m]


def make_templates(Ks, H, W, seed, nonfinite=True):
    """Templates of Ks[j] candidates: left operands of their own, right operands from a shared pool (the finite-delta pairs of a
    frame are shared between templates) plus one of their own; template j is ``make_case(Ks[j], H, W, seed + j)`` with its
    right operands 1.. replaced by the pool's.  The pool's first two entries are one operand, and candidates 1 and 2 tie on a
    third of the pixels.  -> list of (Ls, Rs)."""
    rng = np.random.default_rng([seed, H, W])
    _, pool = make_case(max(max(Ks), 2), H, W, seed + 1000, nonfinite)
    pool[1] = pool[0]
    out = []
    for j, K in enumerate(Ks):
        Ls, Rs = make_case(K, H, W, seed + j, nonfinite)
        if K >= 3:
            _tie(rng, Ls, 1, 2)
        out.append((Ls, Rs[:1] + pool[:K - 1]))
    return out


UP_SHAPES = ((1, 1), (1, 5), (4, 1), (3, 4))
UP_PADS = ((0, 0, 0, 0), (3, 4, 3, 4))
UP_LDS = (3, 4, 7)


def upsample_inputs(P, h, w, ld, seed):
    """flow_lr (P h w, 2), ou (P h w, ld), mask (P h w, 576), float32: mask logits of spread 30 (near one-hot softmaxes),
    occlusion logits of spread 20 (the occlusion saturates to 0 or 1), log-variances in [-60, 80]; the columns of ``ou`` beyond
    the third are NaN -- they are padding and must never reach a result.  The values do not depend on ``ld``."""
    rng = np.random.default_rng([seed, P, h, w])
    M = P * h * w
    flow = (rng.standard_normal((M, 2)) * 4).astype(F32)
    ou = np.full((M, ld), np.nan, F32)
    ou[:, 0:2] = (rng.standard_normal((M, 2)) * 20).astype(F32)
    ou[:, 2] = rng.uniform(-60, 80, M).astype(F32)
    mask = (rng.standard_normal((M, 576)) * 30).astype(F32)
    return flow, ou, mask


# The fp32 oracle (oracle.mft_oracle.convex_upsample + postprocess: ATen's expf, softmax and division on the CPU) against
# upsample_ref on upsample_inputs, every shape / pads / P in {1, 3} above: its worst error, measured by
# tests/test_chain_reference.py::test_oracle_upsample_error_figures (which asserts the figures still hold), in units of
# 2^-24 * max(1, largest neighbour magnitude) -- absolute for the flow (x8 neighbours) and the occlusion (both logits),
# RELATIVE for sigma (log-variance neighbours: sigma = exp(u / 2) turns an absolute error of u into a relative one of sigma).
# The kernel is allowed UP_KERNEL_FACTOR times that: the device's expf and division may round differently from ATen's by a few ulp
# each, while a dropped neighbour, a wrong factor 8 or a wrong crop is orders of magnitude above.
UP_ORACLE_UNITS = {"flow": 3.2, "occl": 0.2, "sigma": 1.4}        # measured: 3.11, 0.198, 1.36
UP_KERNEL_FACTOR = 4.0


def upsample_units(got, ref, N):
    """Worst errors of (flow, occl, sigma) against upsample_ref's float64 results in the units described at UP_ORACLE_UNITS."""
    out = {}
    for name, g, r, n in zip(("flow", "occl", "sigma"), got, ref, N):
        g = np.asarray(g, np.float64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        assert np.isfinite(g).all() and np.isfinite(r).all(), name
        err = np.abs(g - r)
        if name == "sigma":
            err = err / r
        out[name] = float((err / (EPS * np.maximum(1.0, n))).max())
    return out


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------

def units(got, ref, S):
    """The worst error of ``got`` against the float64 ``ref`` in units of 2^-24 * S, over the pixels where ``ref`` is finite;
    raises AssertionError unless ``got`` has NaN exactly where ``ref`` has NaN, and +inf / -inf exactly where ``ref`` has them."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    S = np.broadcast_to(np.asarray(S, np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the reference's"
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)), "+inf pattern differs from the reference's"
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), "-inf pattern differs from the reference's"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - ref[fin])
    s = S[fin]
    assert np.isfinite(s).all()
    # (an exact result where the scale is zero -- every tap outside, a zero left operand -- is no error)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / (EPS * s))
    return float(u.max())


def bits(a):
    """A float32 array (numpy, or a torch tensor on any device) as int32: equality on it tells NaN payloads and signed zeros apart."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------
# the cases of tests/test_gpu_chain_family.py (tests/test_chain_reference.py checks the fp32 oracle on the same ones)
# ---------------------------------------------------------------------------

# (name, Ks of the templates of one chain_select_multi call, H, W, seed)
FAMILY_CASES = (
    ("every-K", tuple(range(1, 17)), 9, 20, 100),                      # KMAX = 16 kernel: 6 templates per launch, three launches
    ("K-to-8", (8, 1, 7, 2, 6, 3, 5, 4, 8, 4, 1, 5, 7), 9, 20, 200),   # KMAX = 8 kernel: 12 per launch, two launches
) + tuple((f"{H}x{W}", KS, H, W, 300 + i) for i, (H, W) in enumerate(SIZES))


def _const(H, W, fx, occl, sigma):
    flow = np.zeros((2, H, W), F32)
    flow[0] = fx
    return flow, np.full((1, H, W), occl, F32), np.full((1, H, W), sigma, F32)


def selection_corners(H=4, W=8):
    """Hand-made candidates: -> list of (name, Ls, Rs, expected chosen index, expected (occl, sigma) of the output or None).
    Candidate k is its left operand (flow 0.25 (k + 1) px in x: exact in float32, stays in the frame) chained with a right
    operand of zeros, which returns it bit for bit -- except where a corner is about the chaining itself."""
    nan, inf = np.nan, np.inf
    zero = _const(H, W, 0.0, 0.0, 0.0)

    def corner(name, occl, sigma, want, Rs=None):
        K = len(occl)
        Ls = [_const(H, W, 0.25 * (k + 1), occl[k], sigma[k]) for k in range(K)]
        return name, Ls, Rs if Rs is not None else [zero] * K, want

    nan_occ_R = _const(H, W, 0.0, nan, 0.0)
    return [
        corner("first NaN sigma wins", [0, 0, 0, 0], [0.5, 0.25, nan, nan], 2),
        corner("NaN sigma under an occlusion above the threshold scores -inf", [0, 0.5, 0], [0.5, nan, 0.375], 2),
        corner("NaN occlusion is not suppressed and is copied out", [0.5, nan, 0.015625], [0.125, 0.25, 0.375], 1),
        corner("+inf sigma everywhere", [0, 0, 0, 0], [inf, inf, inf, inf], 0),
        corner("everything occluded", [0.5, 0.75, 1.0], [0.5, 0.25, 0.125], 0),
        # candidate 0: NaN left occlusion against a finite sample; candidate 1: finite left occlusion against a NaN sample
        corner("NaN on either side of the occlusion maximum", [nan, 0.0, 0.0], [0.25, 0.125, 0.375], 1,
               Rs=[_const(H, W, 0.0, 0.015625, 0.0), nan_occ_R, zero]),
    ]
