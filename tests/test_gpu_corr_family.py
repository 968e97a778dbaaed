"""The correlation family bit for bit against tests/corr_reference.py: the materialised lookup (csrc/motion_front.h), the on-demand
lookup (csrc/corr_ondemand.hip), the lookup fused into convc1 (csrc/lookup_convc1.hip, or csrc/lookup_convc1_wide.hip when the
process loads that library), the volume pyramid in both arithmetics and as the engine builds it, and the feature pyramid.

On the crafted inputs (integer taps of magnitude <= 448, coordinates on the quarter grid: corr_reference's docstring) every
product and partial sum of the blend is exact in float32 and in the 16-bit hi / lo split, so no comparison here has a tolerance:
a wrong tap, weight, channel or mask shows as a plain inequality.  One test (real-valued inputs) uses a derived bound.  Needs an
MI355X."""
import functools

import numpy as np
import pytest
import torch

import corr_reference as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SHAPE_IDS = ["x".join(map(str, s)) for s in cr.SHAPES]


@pytest.fixture(scope="module")
def ops_mod():
    from mft_amd import ops
    return ops


def dev32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def same_bits(got, want):
    """got: float32 device tensor; want: numpy (exact in float32) or a device tensor -> equal bit for bit, zeros compared with ==."""
    want = want if torch.is_tensor(want) else dev32(want)
    got, want = got.contiguous(), want.contiguous().reshape(got.shape)
    return bool(((got.view(torch.int32) == want.view(torch.int32)) | ((got == 0) & (want == 0))).all())


def store_levels(ops, levels, P, h, w, poison=False):
    """Row-major [P * h * w, h_l, w_l] (numpy or device) -> the stored layout [P, h * w, stride_l]; poison: every padding float
    -- block cells beyond w_l and h_l, padded block columns and rows, the stride padding of levels 2 and 3 -- is NaN."""
    out = []
    for l, t in enumerate(levels):
        t = (t if torch.is_tensor(t) else dev32(t)).reshape(P, h * w, (h >> l) * (w >> l))
        s = ops.block_level(t, l, h, w)
        if poison:
            pad = ops.block_level(torch.ones(1, 1, t.shape[-1], device=DEV), l, h, w) == 0
            assert int(pad.sum()) == s.shape[-1] - t.shape[-1]
            s = torch.where(pad, torch.full_like(s, NAN), s)
        out.append(s.contiguous())
    return out


@functools.lru_cache(maxsize=None)
def device_case(P, h, w):
    """corr_reference.exact_case on the device: stored levels (clean and with poisoned padding) and R coordinate sets [P, h * w, 2], each an
    allocation of its own (the kernels want 16-byte aligned operands)."""
    from mft_amd import ops
    case = cr.exact_case(P, h, w)
    lv = store_levels(ops, case["levels"], P, h, w)
    lvp = store_levels(ops, case["levels"], P, h, w, poison=True)
    n_pad = sum(int(torch.isnan(t).sum()) for t in lvp)
    assert n_pad == sum(t.numel() for t in lv) - P * h * w * sum((h >> l) * (w >> l) for l in range(4)) and n_pad > 0
    return {"lv": lv, "lv_poison": lvp, "coords": [dev32(c).reshape(P, h * w, 2) for c in case["coords"]], "want": case["want"]}


@functools.lru_cache(maxsize=None)
def selection_weights():
    """convc1 weights that copy lookup channels: pass 0 output j = channel j, pass 1 output j = channel 68 + j, each with +1 and
    -1 -- relu(v) and relu(-v) together give v, the two passes together all 324 channels.  -> {(pass, sign): fused stream}, bias 0."""
    from mft_amd import ops
    out = {}
    for ps, first in enumerate((0, 68)):
        for sign in (1.0, -1.0):
            wt = torch.zeros(256, 324, 1, 1)
            wt[torch.arange(256), first + torch.arange(256)] = sign
            out[ps, sign] = ops.pack_lookup_convc1_weights(ops.pack_conv_weight(wt.to(DEV)))
    return out, torch.zeros(256, device=DEV)


def fused_lookup(ops, lv, coords, h, w, out_split):
    """All 324 lookup channels [P * h * w, 324] read through corr_lookup_convc1 with the selection weights; also the +1 output
    of pass 0 as the kernel wrote it."""
    wsel, bias = selection_weights()
    halves = []
    for ps in (0, 1):
        pos, neg = (ops.corr_lookup_convc1(lv, coords, h, w, wsel[ps, sign], bias, out_split=out_split) for sign in (1.0, -1.0))
        if out_split:
            pos, neg = ops.unsplit_activations(pos), ops.unsplit_activations(neg)
        if ps == 0:
            raw = pos
        halves.append(pos - neg)                    # one of the two is 0 (or both NaN): exact
    a, b = halves
    ok = (a[:, 68:] == b[:, :188]) | (torch.isnan(a[:, 68:]) & torch.isnan(b[:, :188]))
    assert bool(ok.all()), "channels 68..255 differ between the two passes"
    return torch.cat([a, b[:, 188:]], 1), raw


# ---------------------------------------------------------------------------------------------------------------------------
# a, b: the materialised lookup on crafted levels, clean and with poisoned padding
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned_padding"])
@pytest.mark.parametrize("P,h,w", cr.SHAPES, ids=SHAPE_IDS)
def test_corr_lookup_exact(ops_mod, P, h, w, poison):
    """corr_lookup on the edge coordinates equals lookup_ref bit for bit at every shape; with every padding float of the stored
    levels NaN it returns the same bits (the kernel masks by level size, not by what the padding holds)."""
    c = device_case(P, h, w)
    for r in range(len(c["coords"])):
        got = ops_mod.corr_lookup(c["lv_poison"] if poison else c["lv"], c["coords"][r], h, w)
        assert same_bits(got.reshape(-1, 324), c["want"][r]), (r, _first_diff(got.reshape(-1, 324), c["want"][r]))
        if poison:
            assert same_bits(got, ops_mod.corr_lookup(c["lv"], c["coords"][r], h, w)), r


def _first_diff(got, want):
    """(cell, level, a, b, got, want) of the first mismatch, for the assertion message."""
    got = got.cpu().numpy().astype(np.float64)
    want = np.asarray(want.cpu() if torch.is_tensor(want) else want, np.float64).reshape(got.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    n, ch = bad[0]
    return {"mismatches": len(bad), "cell": int(n), "level": int(ch // 81), "a": int(ch % 81 // 9), "b": int(ch % 9),
            "got": got[n, ch], "want": want[n, ch]}


# ---------------------------------------------------------------------------------------------------------------------------
# c: the fused lookup + convc1 kernel read out through selection weights
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned_padding"])
@pytest.mark.parametrize("P,h,w", cr.SHAPES, ids=SHAPE_IDS)
def test_lookup_convc1_exact(ops_mod, P, h, w, poison):
    """corr_lookup_convc1 with selection weights (output j copies channel j, then channel 68 + j; +1 and -1, zero bias) gives
    lookup_ref's 324 channels bit for bit, as fp32 and in the split form; also with poisoned padding."""
    c = device_case(P, h, w)
    for r in range(len(c["coords"])):
        for out_split in (False, True):
            got, _ = fused_lookup(ops_mod, c["lv_poison"] if poison else c["lv"], c["coords"][r], h, w, out_split)
            assert same_bits(got, c["want"][r]), (r, out_split, _first_diff(got, c["want"][r]))


def test_lookup_convc1_exact_second_tile(ops_mod):
    """7 x 64 x 64 cells: a workgroup of the fused kernel takes a second tile.  The levels are built on the device from the same
    hash; the reference is taken on whole tiles (of 64 and of 56 cells: the first, the last of the first round, the first of the
    second round, the last) and on every 13th cell."""
    P, h, w = cr.LARGE
    N, M = h * w, P * h * w
    lv = []
    for l in range(4):
        hl, wl = h >> l, w >> l
        t = torch.cat([cr.level_values(torch.arange(p * N, (p + 1) * N, device=DEV)[:, None, None], l,
                                       torch.arange(hl, device=DEV)[None, :, None], torch.arange(wl, device=DEV)[None, None, :]).float()
                       for p in range(P)])
        lv.append(t)
    lv = store_levels(ops_mod, lv, P, h, w)
    coords = cr.edge_coords(P, h, w)
    assert coords.shape[0] == 1
    sub = set(range(0, M, 13))
    for tile in (56, 64):
        n_tiles = -(-M // tile)
        for t in (0, n_tiles // 2 - 1, n_tiles // 2, n_tiles - 1):
            sub |= set(range(t * tile, min((t + 1) * tile, M)))
    sub = np.array(sorted(sub))
    assert len(sub) >= 2048 and {0, 55, 256 * 56, 257 * 56 - 1, 511 * 56, M - 1} <= set(sub.tolist())
    want, _ = cr.lookup_ref(cr.crafted_levels(sub, h, w), coords[0][sub])
    cr.assert_exact(want, "expected lookup of the large case")
    cd = dev32(coords[0]).reshape(P, N, 2)
    idx = torch.from_numpy(sub).to(DEV)
    for out_split in (False, True):
        got, _ = fused_lookup(ops_mod, lv, cd, h, w, out_split)
        assert same_bits(got[idx], want), (out_split, _first_diff(got[idx], want))
    assert same_bits(ops_mod.corr_lookup(lv, cd, h, w).reshape(M, 324)[idx], want)


# ---------------------------------------------------------------------------------------------------------------------------
# d: hostile cells among ordinary ones
# ---------------------------------------------------------------------------------------------------------------------------
def _check_hostile(got, clean, want, nan_rows, zero_rows):
    M = got.shape[0]
    assert bool(torch.isnan(got[nan_rows]).all()), "a row with a non-finite coordinate is not NaN in every channel"
    assert bool((got[zero_rows] == 0).all()), "a row with a huge finite coordinate is not 0"
    rest = np.setdiff1d(np.arange(M), np.concatenate([nan_rows, zero_rows]))
    assert same_bits(got[rest], clean[rest]), "a hostile cell changed another row"
    assert same_bits(got[rest], want[rest])


@pytest.mark.parametrize("P,h,w", cr.SHAPES, ids=SHAPE_IDS)
def test_hostile_coordinates(ops_mod, P, h, w):
    """NaN in x only and in y only, +-inf, +-3e9, +-1e30, +-1e6 and the floats next to it, scattered among ordinary cells, for
    corr_lookup, corr_lookup_ondemand and corr_lookup_convc1: non-finite rows are NaN in every channel (all 256 outputs of the
    fused kernel), huge finite rows are 0, every other row has the bits it has without the hostile rows."""
    c = device_case(P, h, w)
    N, M = h * w, P * h * w
    base = cr.exact_case(P, h, w)["coords"][-1]
    hostile, nan_rows, zero_rows = cr.hostile_coords(base)
    want, _ = cr.lookup_ref(cr.exact_case(P, h, w)["levels"], hostile)
    assert np.isnan(want[nan_rows]).all() and (want[zero_rows] == 0).all()
    cb, ch = dev32(base).reshape(P, N, 2), dev32(hostile).reshape(P, N, 2)
    _check_hostile(ops_mod.corr_lookup(c["lv"], ch, h, w).reshape(M, 324), ops_mod.corr_lookup(c["lv"], cb, h, w).reshape(M, 324),
                   want, nan_rows, zero_rows)
    for out_split in (False, True):
        got, raw = fused_lookup(ops_mod, c["lv"], ch, h, w, out_split)
        assert bool(torch.isnan(raw[nan_rows]).all()) and raw.shape[1] == 256
        _check_hostile(got, fused_lookup(ops_mod, c["lv"], cb, h, w, out_split)[0], want, nan_rows, zero_rows)
    f1, f2 = (dev32(f).reshape(P, N, 256) for f in cr.exact_features(P, h, w))
    f2lv = ops_mod.fmap_pyramid(f2, h, w)
    want_od, _ = cr.lookup_ref(cr.pyramid_ref(*cr.exact_features(P, h, w)), hostile)
    _check_hostile(ops_mod.corr_lookup_ondemand(f1, f2lv, ch, h, w).reshape(M, 324),
                   ops_mod.corr_lookup_ondemand(f1, f2lv, cb, h, w).reshape(M, 324), want_od, nan_rows, zero_rows)


# ---------------------------------------------------------------------------------------------------------------------------
# e: the exact feature pair through both pyramids and both lookups
# ---------------------------------------------------------------------------------------------------------------------------
def _check_stored_pyramid(ops, lv, pyr, want_lv, P, h, w, tag):
    """Stored levels against pyramid_ref: every value bit for bit; level 0 whole, i.e. with zeros in its padding -- the padding
    the pyramid's contract specifies (include/mftx.h: the other levels' padding is unspecified, level 1's holds means over level
    0's zero padding; test_corr_lookup_exact and test_lookup_convc1_exact show that no lookup reads any of it)."""
    assert same_bits(lv[0], want_lv[0]), (tag, 0)
    for l in range(4):
        assert same_bits(ops.unblock_level(lv[l], l, h, w).reshape(P * h * w, h >> l, w >> l), pyr[l]), (tag, l)


@pytest.mark.parametrize("P,h,w", cr.SHAPES, ids=SHAPE_IDS)
def test_exact_features_pyramids_and_lookups(ops_mod, P, h, w):
    """f1 = 16 e_k(q), f2 = 64 n: corr_pyramid in both arithmetics equals pyramid_ref bit for bit (level 0's padding zero), fmap_pyramid
    equals feature_pyramid_ref, and corr_lookup / corr_lookup_ondemand on them equal lookup_ref."""
    N, M = h * w, P * h * w
    f1n, f2n = cr.exact_features(P, h, w)
    f1, f2 = dev32(f1n).reshape(P, N, 256), dev32(f2n).reshape(P, N, 256)
    pyr = cr.pyramid_ref(f1n, f2n)
    want_lv = store_levels(ops_mod, pyr, P, h, w)
    coords = cr.exact_case(P, h, w)["coords"]
    wants = []
    for r in range(coords.shape[0]):
        wants.append(cr.lookup_ref(pyr, coords[r])[0])
        cr.assert_exact(wants[-1], "expected lookup on the exact volume")
    for arith in (0, 1):
        lv = ops_mod.corr_pyramid(f1, f2, h, w, arith=arith)
        _check_stored_pyramid(ops_mod, lv, pyr, want_lv, P, h, w, arith)
        for r in range(coords.shape[0]):
            got = ops_mod.corr_lookup(lv, dev32(coords[r]).reshape(P, N, 2), h, w).reshape(M, 324)
            assert same_bits(got, wants[r]), (arith, r, _first_diff(got, wants[r]))
    f2lv = ops_mod.fmap_pyramid(f2, h, w)
    for l, want in enumerate(cr.feature_pyramid_ref(f2n)):
        assert same_bits(f2lv[l], want.reshape(P, -1, 256)), l
    for r in range(coords.shape[0]):
        got = ops_mod.corr_lookup_ondemand(f1, f2lv, dev32(coords[r]).reshape(P, N, 2), h, w).reshape(M, 324)
        assert same_bits(got, wants[r]), (r, _first_diff(got, wants[r]))


@pytest.mark.parametrize("tile_volume", [1, 0])
@pytest.mark.parametrize("P,h,w", [s for s in cr.SHAPES if s[1] >= 16 and s[2] >= 16])
def test_exact_features_engine_volume(ops_mod, P, h, w, tile_volume):
    """The refinement engine's own volume (one iteration; the tile-resident kernel and the ring-buffered GEMM) on the exact
    feature pair, at the shapes the engine accepts (h, w >= 16): pyramid_ref bit for bit, level 0's padding zero."""
    from mft_amd.weights import make_weights
    N = h * w
    f1n, f2n = cr.exact_features(P, h, w)
    f1, f2 = dev32(f1n).reshape(P, N, 256), dev32(f2n).reshape(P, N, 256)
    pyr = cr.pyramid_ref(f1n, f2n)
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in make_weights(7).items()}
    eng = ops_mod.RaftEngine(sd, DEV, options={"tile_volume": tile_volume})
    z = torch.zeros(P, N, 128, device=DEV)
    _, dbg = eng.debug_refine(f1, f2, z, z, h, w, 1)
    stride, _ = ops_mod.pyramid_layout(h, w)
    want_lv = store_levels(ops_mod, pyr, P, h, w)
    for l in range(4):
        got = dbg["costvolume_pyramid"][l]
        assert tuple(got.shape) == (P * N, 1, h >> l, w >> l)
        assert same_bits(got.to(DEV).reshape(P * N, h >> l, w >> l), pyr[l]), l
    _check_stored_pyramid(ops_mod, [eng.region(f"lvl{l}", P, h, w, stride[l]).reshape(P, N, stride[l]) for l in range(4)],
                          pyr, want_lv, P, h, w, tile_volume)


@pytest.mark.parametrize("P,h,w", [s for s in cr.SHAPES if s[1] >= 16 and s[2] >= 16])
def test_exact_features_engine_grouped_lookup(ops_mod, P, h, w):
    """The lookup body inside the grouped lookup + convf1 launch (csrc/raft_engine.hip, schedule "with_lookup"): one iteration
    of the engine on the exact feature pair, started from the edge coordinates through flow_init = coords - grid (exact on the
    quarter grid), leaves lookup_ref's bits in the workspace's lookup features."""
    from mft_amd.weights import make_weights
    N = h * w
    f1n, f2n = cr.exact_features(P, h, w)
    f1, f2 = dev32(f1n).reshape(P, N, 256), dev32(f2n).reshape(P, N, 256)
    pyr = cr.pyramid_ref(f1n, f2n)
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in make_weights(7).items()}
    eng = ops_mod.RaftEngine(sd, DEV, options={"fuse_lookup": 0, "fuse_flow": 0, "fork": 0})
    assert eng.plan(P, h, w)["flow"] == "with_lookup"
    z = torch.zeros(P, N, 128, device=DEV)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    grid = np.tile(np.stack([xs.ravel(), ys.ravel()], 1), (P, 1))
    for r, coords in enumerate(cr.exact_case(P, h, w)["coords"]):
        flow_init = coords - grid
        assert np.array_equal(grid + flow_init, coords)
        eng.refine(f1, f2, z, z, h, w, 1, flow_init=dev32(flow_init).reshape(P, N, 2))
        want, _ = cr.lookup_ref(pyr, coords)
        got = eng.region("corr", P, h, w, 324)
        assert same_bits(got, want), (r, _first_diff(got, want))


# ---------------------------------------------------------------------------------------------------------------------------
# f: batch invariance; g: real-valued inputs against the derived bound
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_case(P, h, w, seed):
    rng = np.random.default_rng(seed)
    levels = [rng.standard_normal((P * h * w, h >> l, w >> l)).astype(np.float32) for l in range(4)]
    edge = cr.edge_coords(P, h, w)[0]
    coords = (edge.astype(np.float64) + rng.standard_normal(edge.shape) * 0.37).astype(np.float32)      # off the quarter grid
    return levels, coords


def test_lookup_rows_independent_of_batch(ops_mod):
    """At 3 x 17 x 23 each pair looked up alone equals its slice of the batched call, bit for bit, for the materialised and the
    on-demand lookup, on real-valued inputs (the fused kernel: test_lookup_convc1_fused_batch_and_tile_invariance)."""
    P, h, w = 3, 17, 23
    N = h * w
    levels, coords = _gauss_case(P, h, w, seed=31)
    lv = store_levels(ops_mod, levels, P, h, w)
    cd = dev32(coords).reshape(P, N, 2)
    whole = ops_mod.corr_lookup(lv, cd, h, w)
    g = torch.Generator().manual_seed(32)
    f1, f2 = (torch.randn(P, N, 256, generator=g).to(DEV) for _ in range(2))
    f2lv = ops_mod.fmap_pyramid(f2, h, w)
    whole_od = ops_mod.corr_lookup_ondemand(f1, f2lv, cd, h, w)
    assert bool(torch.isfinite(whole).all()) and bool(torch.isfinite(whole_od).all())
    for i in range(P):
        ci = cd[i:i + 1].contiguous()
        one = ops_mod.corr_lookup([t[i:i + 1].contiguous() for t in lv], ci, h, w)
        assert torch.equal(one[0].view(torch.int32), whole[i].view(torch.int32)), i
        one = ops_mod.corr_lookup_ondemand(f1[i:i + 1].contiguous(), [t[i:i + 1].contiguous() for t in f2lv], ci, h, w)
        assert torch.equal(one[0].view(torch.int32), whole_od[i].view(torch.int32)), i


@pytest.mark.parametrize("P,h,w", cr.SHAPES, ids=SHAPE_IDS)
def test_corr_lookup_real_valued_within_derived_bound(ops_mod, P, h, w):
    """Gaussian levels, the edge coordinates perturbed off the quarter grid: |got - lookup_ref| <= 8 * 2^-24 * mag per output,
    mag = sum |w_i| |t_i|.  Derived, not tuned: one rounding each for 1 - fx, 1 - fy and the weight product (3 units per weight),
    four products and three additions (at most 4 more), one unit left over; a fused multiply-add only lowers the error.
    Measured on an MI355X: the kernel uses 0.382 of the bound at most, at 2 x 9 x 15."""
    levels, coords = _gauss_case(P, h, w, seed=41)
    want, mag = cr.lookup_ref(levels, coords)
    got = ops_mod.corr_lookup(store_levels(ops_mod, levels, P, h, w), dev32(coords).reshape(P, h * w, 2), h, w)
    err = np.abs(got.reshape(-1, 324).cpu().numpy().astype(np.float64) - want)
    bound = cr.LOOKUP_BOUND_UNITS * cr.EPS * mag
    print(f"corr_lookup {P}x{h}x{w}: largest share of the 8 EPS mag bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
