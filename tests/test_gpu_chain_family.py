"""Every variant of the chaining, selection and read-out kernels (csrc/chain.hip) and the upsampler that feeds them
(csrc/upsample.hip) against exact references in plain numpy (tests/chain_reference.py, pinned on the CPU by
tests/test_chain_reference.py), inf and NaN included.  Needs an MI355X.

WHAT IS COMPARED, per case
  1. ``ops.chain(L_k, R_k)`` against ``chain_ref`` (float32 sampling coordinates, everything else float64), every candidate,
     within BOUND units of 2^-24 S; NaN exactly where the reference has NaN, +-inf where it has +-inf.
  2. ``ops.select`` on those chained candidates against ``select_ref`` on the DOWNLOADED candidates: flow, occlusion, sigma and
     the chosen index bit for bit at every pixel (the selection is exact given its candidates).
  3. ``ops.chain_select``, ``ops.chain_select_packed``, ``ops.chain_select_multi`` (the case as one template among others) and,
     where W % 4 == 0, the same calls with operands based 4 bytes off a 16-byte boundary (the one-pixel ``select_kernel``
     instead of ``select4_kernel``): each bit for bit equal to step 2.
  Floats that may be NaN are compared as int32.

THE BOUND of step 1: |got - ref| <= 12 * 2^-24 * S, with S per pixel = |px| + |g| + max|tap| for a flow component (px = x + the
left flow, g = x) and the largest magnitude involved for occlusion and sigma.  Derivation, every rounding counted at its worst
(relative error u = 2^-24 per float32 operation; m = max|tap|):
  * The coordinates, floor and the fraction w = ix - floor(ix) are float32 in the reference too: no error.  A weight carries the
    rounding of at most two subtractions (1 - wx, 1 - wy) and one product: relative error at most 3 u, and 2 u on average over
    the four weights ((1 - wx)(1 - wy): 3, wx (1 - wy) and (1 - wx) wy: 2, wx wy: 1).
  * A sample is four products tap * weight (1 u each) and three sums (1 u each, of partial sums no larger than m, the weights
    summing to one): at most (3 + 1) u m from the terms, where the term of weight-error 3 has it only when its weight is not
    near 1, and 3 u m from the sums -- 6 u m by the issue's count, 7 u m counting every rounding at its worst.
  * A flow component adds (px + sample) and subtracts g, two more roundings of magnitudes below S: at most 8 (9) u S.  The
    occlusion is a maximum, which is exact: 6 (7) u S.
  * Sigma = sqrt(sl^2 + sr^2): an error d of the sample sr moves it by d sr / sigma <= d, the two squares and the sum add at most
    1.5 u sigma, a correctly rounded square root u / 2: at most 9 (10) u S.
  * 12 therefore holds even by the cruder count, with 2 u of headroom for the one thing reading cannot settle: whether ``sqrtf``
    is correctly rounded under the build's flags.
  The fp32 CPU oracle -- the kernel's operation order, independently written -- stays within 2.8 (flow), 2.9 (occlusion) and 3.2
  (sigma) units on exactly these inputs (tests/test_chain_reference.py::test_oracle_chain_within_the_gpu_bound).
  Measured on an MI355X: the kernels' worst errors here are 2.75 (flow), 2.89 (occlusion) and 2.95 (sigma) units.

THE UPSAMPLER'S BOUND depends on the accuracy of the device's expf, so it is anchored to a measurement of the REFERENCE side: the
fp32 oracle (ATen's expf, softmax, division) against ``upsample_ref`` (float64) on exactly these inputs is off by at most 3.11
(flow), 0.198 (occlusion) and 1.36 (sigma, relative) units of 2^-24 * max(1, largest neighbour magnitude) -- recorded as
3.2 / 0.2 / 1.4 in chain_reference.UP_ORACLE_UNITS and re-measured by test_chain_reference.py::test_oracle_upsample_error_figures.
The kernel is allowed 4 x that: 12.8 / 0.8 / 5.6 units.  A dropped neighbour, a wrong x8 or a wrong crop is orders of magnitude above.
Measured on an MI355X: the kernel's worst errors here are 3.11 / 0.198 / 1.36 units -- the oracle's own.

WHERE EACH PATH IS COVERED
  * chain_kernel, chain_select_kernel, select_kernel / select4_kernel: K = 1..16 at 9 x 20 (W % 4 == 0: both select kernels);
    K in {1, 4, 5, 8, 9, 16} at 2 x 2 (the minimum), 5 x 4 (one float4 per row), 3 x 259 (a second block of 3 pixels; scalar
    select), 2 x 260 (select4 across the block seam: 64 threads x 4 pixels, then one more thread), 37 x 53 (odd, unaligned planes).
  * chain_select_packed_kernel<KT>: KT = 1..8 and KT = 0 at K = 9..16, all at 9 x 20; KT in {1, 4, 5, 8} and KT = 0 at
    K in {9, 16} at the five sizes above.
  * chain_select_multi_kernel<16, 6>: sixteen templates of K = 1..16 in one call (three launches) at 9 x 20; six templates of
    K in {1, 4, 5, 8, 9, 16} at the five sizes.  <8, 12>: thirteen templates of K <= 8 (two launches) at 9 x 20; the four
    templates of K <= 8 at the five sizes.
  * the selection rule's corners (first NaN wins, NaN under occlusion, NaN occlusion, all +inf, all occluded, NaN on either side of
    the occlusion maximum): hand-made candidates at 4 x 8, K = 3..4, through every variant above.
  * sample_points_kernel: 130 templates of 5 x 7 (two launches: t0 = 0 and t0 = 128, template ids 0, 1, 127, 128, 129, and the ids
    130 and -1 that must leave their rows alone), and 3 templates of 37 x 53.
  * warp_backward_kernel: C in {1, 2, 3, 5} at 2 x 2, 7 x 259, 37 x 53, every channel.
  * convex_upsample_kernel: P in {1, 3} x ld_ou in {3, 4, 7} x (h, w) in {(1, 1), (1, 5), (4, 1), (3, 4)} x pads in
    {(0, 0, 0, 0), (3, 4, 3, 4)}, planar and packed.
  * one sampler across sample_points_kernel, warp_backward_kernel and chain_kernel (csrc/grid_sample.h): bit for bit on one right
    result at 5 x 7 and 37 x 53, every class of ``_point_kinds`` among the destinations.

None of these inputs can produce an out-of-range address: the clamps of the tap coordinates precede the int cast, ``tap()`` checks
bounds before it reads and ``clamped_tap()`` (under ``packed_tap()``) clamps the address.  These are value tests."""
import numpy as np
import pytest
import torch

import chain_reference as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 12.0
THR = cr.THR
PARTS = ("flow", "occlusion", "sigma", "chosen")
WORST = {}            # the worst error met so far, per quantity, in the units of its bound (printed: run with -s to see the figures)


@pytest.fixture(scope="module")
def ops():
    from mft_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def misaligned(t):                       # same values, base address 4 bytes off a 16-byte boundary
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def same_bits(a, b):
    """Bitwise equality of two tensors (float32 compared as int32: torch.equal is false on NaN)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def assert_same(got, want, what):
    for part, a, b in zip(PARTS, got, want):
        assert same_bits(a, b), (what, part, int((a.contiguous().view(-1) != b.contiguous().view(-1)).sum()))


class Uploads:
    """numpy operands -> device operands, each distinct array once (templates share right operands: the same device tensor)."""

    def __init__(self):
        self.planar, self.packed = {}, {}

    def result(self, res):
        key = id(res[0])
        if key not in self.planar:
            self.planar[key] = (res, tuple(dev(a) for a in res))       # (the numpy triple is kept alive: ids stay unique)
        return self.planar[key][1]

    def pack(self, res):
        key = id(res[0])
        if key not in self.packed:
            self.packed[key] = (res, dev(np.concatenate(res, 0).transpose(1, 2, 0)))
        return self.packed[key][1]


def run_template(ops, up, Ls, Rs, what):
    """Steps 1 to 3 for one template's candidates; -> the result of step 2 (device tensors: flow, occl, sigma, chosen)."""
    _, H, W = Ls[0][0].shape
    dL, dR = [up.result(L) for L in Ls], [up.result(R) for R in Rs]
    # 1: every chained candidate against the reference
    chained = [ops.chain(l, r) for l, r in zip(dL, dR)]
    for k, (c, L, R) in enumerate(zip(chained, Ls, Rs)):
        ref, S = cr.chain_ref(L, R)
        for part, g, r, s in zip(PARTS, c, ref, S):
            u = cr.units(g.cpu().numpy(), r, s)
            WORST[part] = max(WORST.get(part, 0.0), u)
            assert u <= BOUND, (what, k, part, u)
    # 2: the selection, exact given the GPU's own candidates
    sel = ops.select(chained, THR, want_chosen=True)
    want = cr.select_ref([tuple(t.cpu().numpy() for t in c) for c in chained], THR)
    for part, g, r in zip(PARTS, sel, want):
        g = g.cpu().numpy()
        assert g.shape == r.shape, (what, part)
        bad = cr.bits(g) != cr.bits(r.astype(g.dtype))
        assert not bad.any(), (what, part, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # 3: the fused variants
    packed = [up.pack(R) for R in Rs]
    assert_same(ops.chain_select(dL, dR, THR, want_chosen=True), sel, (what, "chain_select"))
    assert_same(ops.chain_select_packed(dL, packed, THR, want_chosen=True), sel, (what, "chain_select_packed"))
    no_chosen = ops.chain_select_packed(dL, packed, THR)
    assert no_chosen[3] is None
    assert_same(no_chosen[:3], sel[:3], (what, "chain_select_packed without chosen"))
    if W % 4 == 0:
        mL = [tuple(misaligned(t) for t in l) for l in dL]
        mR = [tuple(misaligned(t) for t in r) for r in dR]
        assert_same(ops.select([tuple(misaligned(t) for t in c) for c in chained], THR, want_chosen=True), sel, (what, "select, misaligned"))
        assert_same(ops.chain_select(mL, mR, THR, want_chosen=True), sel, (what, "chain_select, misaligned"))
        assert_same(ops.chain_select_packed(mL, packed, THR, want_chosen=True), sel, (what, "chain_select_packed, misaligned"))
    return sel


def run_templates(ops, templates, what):
    """Steps 1 to 3 for every template, then all of them as one chain_select_multi call -- and, where some have more than 8
    candidates, those with at most 8 as a call of their own (the batched-tap multi kernel)."""
    up = Uploads()
    sels = [run_template(ops, up, Ls, Rs, (what, j, len(Ls))) for j, (Ls, Rs) in enumerate(templates)]
    groups = [list(range(len(templates)))]
    small = [j for j, (Ls, _) in enumerate(templates) if len(Ls) <= 8]
    if 0 < len(small) < len(templates):
        groups.append(small)
    for grp in groups:
        multi = ops.chain_select_multi([([up.result(L) for L in templates[j][0]], [up.pack(R) for R in templates[j][1]]) for j in grp],
                                       THR, want_chosen=True)
        assert len(multi) == len(grp)
        for j, m in zip(grp, multi):
            assert_same(m, sels[j], (what, "chain_select_multi", len(grp), j, len(templates[j][0])))
    return sels


@pytest.mark.parametrize("case", cr.FAMILY_CASES, ids=[c[0] for c in cr.FAMILY_CASES])
def test_chain_family(ops, case):
    name, Ks, H, W, seed = case
    templates = cr.make_templates(Ks, H, W, seed)
    assert templates[-1][1][1] is templates[-2][1][1]                  # right operands are shared between templates
    sels = run_templates(ops, templates, name)
    print(f"chain against chain_ref up to {name}: worst error in units of 2^-24 S:", {k: round(WORST[k], 2) for k in PARTS[:3]})
    # the inputs do exercise what they are meant to: NaN and inf reach the outputs, several candidates win, flows leave the frame
    occ = torch.stack([s[1] for s in sels]).cpu().numpy()
    sig = torch.stack([s[2] for s in sels]).cpu().numpy()
    if H * W >= 100:
        assert np.isnan(occ).any() and np.isnan(sig).any() and np.isposinf(sig).any() and (occ == 1).any()
        assert all(len(torch.unique(s[3])) >= min(len(t[0]), 3) for s, t in zip(sels, templates))


def test_selection_corners(ops):
    corners = cr.selection_corners()
    sels = run_templates(ops, [(Ls, Rs) for _, Ls, Rs, _ in corners], "corners")
    for (name, Ls, Rs, k), sel in zip(corners, sels):
        assert bool((sel[3] == k).all()), name
        for part, a, b in zip(PARTS[1:3], sel[1:3], Ls[k][1:3]):      # the chosen candidate's occlusion and sigma are copied out
            if "either side" not in name:
                assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), (name, part)
    by_name = {c[0]: s for c, s in zip(corners, sels)}
    assert bool(torch.isnan(by_name["NaN occlusion is not suppressed and is copied out"][1]).all())
    assert bool(torch.isnan(by_name["first NaN sigma wins"][2]).all())
    assert bool(torch.isnan(by_name["NaN on either side of the occlusion maximum"][1]).all())
    # max_nanprop: a NaN on either side of the maximum gives NaN (chain_ref says the same: step 1 above)
    name, Ls, Rs, _ = corners[-1]
    for k in (0, 1):
        assert bool(torch.isnan(ops.chain(tuple(dev(a) for a in Ls[k]), tuple(dev(a) for a in Rs[k]))[1]).all()), k


# ---------------------------------------------------------------------------
# point read-out
# ---------------------------------------------------------------------------

def _point_kinds(H, W):
    """Interior fractional; exactly integral; exactly (W - 1, H - 1); outside by less than a pixel on each side; outside by more
    than a pixel; +-1e5; +-3e9."""
    return np.array([(1.25, 2.5), (W - 2.75, 0.125), (0.0625, H - 1.5), (2.0, 1.0), (0.0, 0.0), (W - 1, H - 1), (1.0, H - 1),
                     (-0.5, 1.5), (W - 0.25, 2.0), (2.5, -0.75), (1.0, H - 0.5), (-0.5, -0.5), (W - 0.5, H - 0.5),
                     (-1.5, 1.0), (W + 0.75, 2.25), (3.0, -2.5), (2.5, H + 1.0), (-3.0, H + 3.0),
                     (1e5, 1.0), (2.0, -1e5), (-1e5, 1e5), (3e9, 2.0), (1.5, -3e9), (-3e9, 3e9)], np.float32)


@pytest.mark.parametrize("T,H,W,ids", [(130, 5, 7, (0, 1, 5, 64, 127, 128, 129)), (3, 37, 53, (0, 1, 2))],
                         ids=["130-templates-5x7", "3-templates-37x53"])
def test_sample_points(ops, T, H, W, ids):
    rng = np.random.default_rng([9, T, H, W])
    results = [cr.make_result(rng, H, W, 3.0, False, True) for _ in range(T)]
    kinds = _point_kinds(H, W)
    more = np.stack([rng.uniform(-2, W + 1, 40), rng.uniform(-2, H + 1, 40)], 1).astype(np.float32)
    pts = np.concatenate([kinds, more])
    tmpl = np.repeat(np.array(ids + (T, -1), np.int32), len(pts))      # (ids T and -1: no such template, their rows stay)
    xy = np.tile(pts, (len(ids) + 2, 1))
    order = rng.permutation(len(tmpl))                                 # templates interleaved across the launch's blocks
    tmpl, xy = tmpl[order], np.ascontiguousarray(xy[order])
    N = len(tmpl)
    assert N > 256 or T < 128                                          # more than one block
    sentinel = np.float32(-7.25)
    table = torch.full((N, 3, 4), float(sentinel), device=DEV)
    ops.sample_points([tuple(dev(a) for a in r) for r in results], dev(tmpl), dev(xy), table, 1)
    t = table.cpu().numpy()
    assert np.array_equal(cr.bits(t[:, [0, 2]]), cr.bits(np.full((N, 2, 4), sentinel)))       # the other columns keep every bit
    absent = (tmpl == T) | (tmpl == -1)
    assert absent.sum() == 2 * len(pts)
    assert np.array_equal(cr.bits(t[absent, 1]), cr.bits(np.full((int(absent.sum()), 4), sentinel)))
    for j in ids:
        m = tmpl == j
        got = t[m, 1]                                                  # (x + flow x, y + flow y, occlusion, sigma)
        flow, occl, sigma = results[j]
        (sf, bf), (so, bo), (ss, bs) = (cr.sample_ref(p, xy[m]) for p in (flow, occl, sigma))
        p64 = xy[m].astype(np.float64)
        for c in (0, 1):
            u = cr.units(got[:, c], p64[:, c] + sf[c], np.abs(p64[:, c]) + bf[c])
            assert u <= BOUND, (j, "xy"[c], u)
        for name, g, r, s in (("occlusion", got[:, 2], so[0], bo[0]), ("sigma", got[:, 3], ss[0], bs[0])):
            u = cr.units(g, r, s)
            assert u <= BOUND, (j, name, u)


# ---------------------------------------------------------------------------
# warp_backward
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(2, 2), (7, 259), (37, 53)])
@pytest.mark.parametrize("C", [1, 2, 3, 5])
def test_warp_backward(ops, C, H, W):
    """Every channel against the reference sampler at p = grid + flow (float32 sum, as in the kernel); flows leave the frame,
    the image holds NaN and +-inf on its border."""
    rng = np.random.default_rng([10, C, H, W])
    flow = cr.make_result(rng, H, W, 3.0, True, False)[0]
    img = (rng.standard_normal((C, H, W)) * 5).astype(np.float32)
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    pick = np.where(border[None], rng.random((C, H, W)), 1.0)
    img[pick < 0.1] = np.nan
    img[(pick >= 0.1) & (pick < 0.2)] = np.inf
    img[(pick >= 0.2) & (pick < 0.3)] = -np.inf
    got = ops.warp_backward(dev(flow), dev(img)).cpu().numpy()
    gx, gy = cr._grid(H, W)
    ref, S = cr.sample_at(img, gx + flow[0], gy + flow[1])
    assert got.shape == (C, H, W)
    for c in range(C):
        u = cr.units(got[c], ref[c], S[c])
        assert u <= BOUND, (c, u)
    if H * W > 100:
        assert (~np.isfinite(ref)).any() and (np.isfinite(ref) & (ref != 0)).mean() > 0.25


# ---------------------------------------------------------------------------
# one sampler across the kernels
# ---------------------------------------------------------------------------

def _same_or_both_nan(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(got) | np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    bad = (cr.bits(got) != cr.bits(want)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("H,W", [(5, 7), (37, 53)])
def test_one_sampler_across_kernels(ops, H, W):
    """``sample_points``, ``warp_backward`` and ``chain`` sample one right result R at the same destinations g + flow and must
    give the same bits: they share one sampler (csrc/grid_sample.h).  The destinations cover every class of ``_point_kinds``;
    R holds NaN and +inf.  Compared as int32; where one side is NaN only "both are NaN" is asserted.  (The track store's query is
    tied to ``sample_points`` by tests/test_gpu_trackstore.py.)  Sigma of ``chain`` is not compared: sqrt(sr * sr) is not sr."""
    rng = np.random.default_rng([11, H, W])
    R = cr.make_result(rng, H, W, 3.0, False, True)
    flow = cr.make_result(rng, H, W, 3.0, True, False)[0]
    gx, gy = cr._grid(H, W)
    kinds = _point_kinds(H, W)
    n = len(kinds)
    assert n <= H * W
    flat = flow.reshape(2, -1)
    flat[0, :n] = kinds[:, 0] - gx.reshape(-1)[:n]
    flat[1, :n] = kinds[:, 1] - gy.reshape(-1)[:n]
    px, py = gx + flow[0], gy + flow[1]                                # float32: the one IEEE addition the kernels do
    assert px.dtype == np.float32 and py.dtype == np.float32
    assert np.array_equal(np.stack([px.reshape(-1)[:n], py.reshape(-1)[:n]], 1), kinds)      # every class is met as written
    N = H * W
    # 1: sample_points, the anchor
    xy = np.stack([px.reshape(-1), py.reshape(-1)], 1)
    table = torch.zeros((N, 4), device=DEV)
    ops.sample_points([tuple(dev(a) for a in R)], torch.zeros(N, dtype=torch.int32, device=DEV), dev(xy), table, 0)
    row = table.cpu().numpy().reshape(H, W, 4)
    s_occl, s_sigma = row[..., 2], row[..., 3]
    # 2: warp_backward of the stacked planes (occlusion, sigma)
    warped = ops.warp_backward(dev(flow), dev(np.concatenate([R[1], R[2]], 0))).cpu().numpy()
    _same_or_both_nan(warped[0], s_occl, "warp_backward, occlusion plane")
    _same_or_both_nan(warped[1], s_sigma, "warp_backward, sigma plane")
    # 3: chain behind a left result that leaves the right one as it is (max(-inf, o) = o)
    L = (flow, np.full((1, H, W), -np.inf, np.float32), np.zeros((1, H, W), np.float32))
    cflow, coccl, _ = (t.cpu().numpy() for t in ops.chain(tuple(dev(a) for a in L), tuple(dev(a) for a in R)))
    _same_or_both_nan(coccl[0], s_occl, "chain, occlusion")
    with np.errstate(invalid="ignore", over="ignore"):
        want_fx, want_fy = row[..., 0] - gx, row[..., 1] - gy
    assert want_fx.dtype == np.float32
    _same_or_both_nan(cflow[0], want_fx, "chain, flow x")
    _same_or_both_nan(cflow[1], want_fy, "chain, flow y")
    # the inputs do exercise the sampler: taps inside and outside, and non-finite samples at the larger size
    assert (s_sigma == 0).any() and (np.isfinite(s_sigma) & (s_sigma != 0)).any()
    if H * W > 100:
        assert np.isnan(s_sigma).any() and np.isposinf(s_sigma).any()


# ---------------------------------------------------------------------------
# convex upsampling
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", cr.UP_SHAPES)
@pytest.mark.parametrize("P", [1, 3])
def test_convex_upsample(ops, P, h, w):
    """Against upsample_ref (float64) within 4 x the fp32 oracle's own error on these inputs: 12.8 (flow), 0.8 (occlusion) and
    5.6 (sigma, relative) units of 2^-24 * max(1, largest neighbour magnitude) -- the oracle's measured 3.11 / 0.198 / 1.36,
    recorded as 3.2 / 0.2 / 1.4.  Planar == packed, any ld_ou gives the same bits (the NaN padding columns are never read), and
    every pair of a P = 3 call equals the pair run alone, bit for bit."""
    for pads in cr.UP_PADS:
        base = None
        for ld in cr.UP_LDS:
            flow_lr, ou, mask = cr.upsample_inputs(P, h, w, ld, seed=7)
            assert ld == 3 or np.isnan(ou[:, 3:]).all()
            d = [dev(a) for a in (flow_lr, ou, mask)]
            flow, occl, sigma, packed = ops.convex_upsample(*d, P, h, w, pads=pads, want_packed=True)
            plain = ops.convex_upsample(*d, P, h, w, pads=pads)
            assert_same(plain, (flow, occl, sigma), (pads, ld, "planar alone"))
            assert same_bits(packed, torch.cat([flow, occl, sigma], 1).permute(0, 2, 3, 1).contiguous()), (pads, ld, "packed")
            if base is None:
                base = (flow, occl, sigma)
                ref, N = cr.upsample_ref(flow_lr, ou, mask, P, h, w, pads)
                u = cr.upsample_units([t.cpu().numpy() for t in base], ref, N)
                print(f"convex_upsample P={P} {h}x{w} pads={pads}: error in units of 2^-24 max(1, neighbour):", {k: round(v, 3) for k, v in u.items()})
                for k in u:
                    assert u[k] <= cr.UP_KERNEL_FACTOR * cr.UP_ORACLE_UNITS[k], (pads, k, u[k])
            else:
                assert_same((flow, occl, sigma), base, (pads, ld, "ld_ou"))
            if P > 1:
                M = h * w
                for p in range(P):
                    one = ops.convex_upsample(*[t[p * M:(p + 1) * M].contiguous() for t in d], 1, h, w, pads=pads)
                    assert_same([t[0] for t in one], [t[p] for t in (flow, occl, sigma)], (pads, ld, "pair alone", p))
