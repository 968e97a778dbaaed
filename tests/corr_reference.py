"""Exact references, in plain numpy, for the correlation family -- the volume pyramid (csrc/corr.hip, csrc/volume_tile.hip), the
feature pyramid and the lookups in their five forms (csrc/motion_front.h alone and in the grouped launch, csrc/corr_ondemand.hip,
csrc/lookup_convc1.hip, csrc/lookup_convc1_wide.hip) -- TEST INFRASTRUCTURE.

The definition of the lookup the kernels and this module share (core/corr.py:30-51 without grid_sample's normalise round trip):

* The coordinate arithmetic is float32, operation by operation as the kernels state it: ``s = c / 2^l`` (exact), ``floor(s)``,
  ``f = s - floor(s)``; the four bilinear weights are float32 products of ``1 - f`` and ``f``.
* Everything after that is float64.  The window of level l starts at ``floor(s) - 4`` and is 10 x 10 taps; a tap outside the level
  is 0 whatever the stored level holds there; a tap inside takes part even at zero weight.  Output channel ``l * 81 + a * 9 + b``
  is the sample at window column a (x), row b (y).
* A non-finite coordinate gives NaN weights (``inf - inf``), hence NaN in all 324 channels; a huge finite one gives weights
  (1, 0, 0, 0) or the like on taps that are all outside: 0.

INPUTS ON WHICH THE ARITHMETIC IS EXACT.  With integer taps of magnitude <= 448 and coordinates that are multiples of 1/4, every
weight at every level is a multiple of 2^-10, every product and every partial sum of the blend fits 19 bits: the float32 blend in
any summation order, with or without contraction, equals the float64 value, and so does its 16-bit split ``hi + lo / 2048``.  On
such inputs every lookup variant must return this module's bits.  One stage earlier: ``f1[q] = 16 e_k(q)`` and ``f2[p][c] = 64 n``,
integer ``|n| <= 7``, make the volume ``<f1, f2> / 16`` the integer table ``f2[p][k(q)]`` and every pooled level (of the volume and of
the feature map) a mean of multiples of 64 -- integers, so both pyramids are exact too.  The builders below assert these
conditions on what they return.

tests/test_corr_reference.py pins this module against torch and the oracle on the CPU."""
import functools

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24           # half an ulp of 1.0f: the relative rounding error of one fp32 operation
LOOKUP_BOUND_UNITS = 8     # |fp32 blend - lookup_ref| <= 8 EPS mag: 3 per weight (1 - fx, 1 - fy, their product), 4 products + 3 sums <= 4, 1 spare

# (P, h, w) of tests/test_gpu_corr_family.py
SHAPES = [(1, 8, 8),       # level 3 is 1 x 1; strides of levels 2 and 3 are padding only
          (2, 9, 15),      # one super-block; widths 15, 7, 3, 1
          (1, 17, 23),     # 391 cells, odd: the tail of the two-cells-per-wave loop
          (3, 17, 23),     # the same grid with three pairs
          (1, 16, 24),     # aligned
          (1, 12, 33)]     # widths 33, 16, 8, 4
LARGE = (7, 64, 64)        # the fused kernel's workgroups take a second tile


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _window_origin(fl):
    """``(int)fminf(fmaxf(floorf(s), -1e6), 1e6) - 4``: fmaxf drops a NaN, beyond +-1e6 every tap is outside any level."""
    with np.errstate(invalid="ignore"):
        fl = np.where(np.isnan(fl), F32(-1.0e6), np.clip(fl, F32(-1.0e6), F32(1.0e6)))
    return fl.astype(np.int64) - 4


def lookup_weights(coords, l):
    """-> (x0, y0 int64 window origins, (w00, w01, w10, w11) float32) of level l; w01 weighs the tap one column to the right."""
    c = np.ascontiguousarray(coords, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = c[:, 0] / F32(1 << l), c[:, 1] / F32(1 << l)
        flx, fly = np.floor(sx), np.floor(sy)
        fx, fy = sx - flx, sy - fly
        gx, gy = F32(1) - fx, F32(1) - fy
        w = (gx * gy, fx * gy, gx * fy, fx * fy)
    assert all(t.dtype == F32 for t in w)
    return _window_origin(flx), _window_origin(fly), w


def window_patches(level, x0, y0):
    """level [N, H, W] -> the 10 x 10 windows [N, 10 (row), 10 (column)] in float64, zeros outside the level."""
    N, H, W = level.shape
    ys = y0[:, None] + np.arange(10)
    xs = x0[:, None] + np.arange(10)
    iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    t = level[np.arange(N)[:, None, None], np.clip(ys, 0, H - 1)[:, :, None], np.clip(xs, 0, W - 1)[:, None, :]]
    return np.where(iy[:, :, None] & ix[:, None, :], t.astype(np.float64), 0.0)


def lookup_ref(levels, coords):
    """levels: four row-major arrays [N, h_l, w_l] (cell n's own slice of level l); coords [N, 2] float32 (x, y).
    -> (values float64 [N, 324], mag float64 [N, 324] = sum |w_i| |t_i| per output)."""
    N = coords.shape[0]
    out = np.empty((N, 4, 9, 9), np.float64)          # [n, l, a, b]
    mag = np.empty((N, 4, 9, 9), np.float64)
    for l, level in enumerate(levels):
        assert level.shape[0] == N
        x0, y0, w = lookup_weights(coords, l)
        t = window_patches(np.asarray(level), x0, y0)
        w00, w01, w10, w11 = (v.astype(np.float64)[:, None, None] for v in w)
        with np.errstate(invalid="ignore"):
            v = w00 * t[:, :9, :9] + w01 * t[:, :9, 1:] + w10 * t[:, 1:, :9] + w11 * t[:, 1:, 1:]       # [n, b, a]
            m = np.abs(w00) * np.abs(t[:, :9, :9]) + np.abs(w01) * np.abs(t[:, :9, 1:]) \
                + np.abs(w10) * np.abs(t[:, 1:, :9]) + np.abs(w11) * np.abs(t[:, 1:, 1:])
        out[:, l] = v.transpose(0, 2, 1)
        mag[:, l] = m.transpose(0, 2, 1)
    return out.reshape(N, 324), mag.reshape(N, 324)


def lookup_f32(levels, coords):
    """The same blend in plain float32 numpy, products summed left to right (no FMA): what the 8 EPS mag bound is about."""
    N = coords.shape[0]
    out = np.empty((N, 4, 9, 9), F32)
    for l, level in enumerate(levels):
        x0, y0, (w00, w01, w10, w11) = lookup_weights(coords, l)
        t = window_patches(np.asarray(level), x0, y0).astype(F32)
        w00, w01, w10, w11 = (v[:, None, None] for v in (w00, w01, w10, w11))
        with np.errstate(invalid="ignore"):
            v = ((w00 * t[:, :9, :9] + w01 * t[:, :9, 1:]) + w10 * t[:, 1:, :9]) + w11 * t[:, 1:, 1:]
        assert v.dtype == F32
        out[:, l] = v.transpose(0, 2, 1)
    return out.reshape(N, 324)


def _pool(a, ay, ax):
    """Floor-sized 2 x 2 mean over axes (ay, ax), float64."""
    H2, W2 = a.shape[ay] // 2, a.shape[ax] // 2
    def cut(oy, ox):
        s = [slice(None)] * a.ndim
        s[ay], s[ax] = slice(oy, 2 * H2, 2), slice(ox, 2 * W2, 2)
        return a[tuple(s)]
    return (cut(0, 0) + cut(0, 1) + cut(1, 0) + cut(1, 1)) * 0.25


def pyramid_ref(f1, f2):
    """f1, f2 [P, h, w, C] -> four levels [P * h * w, h_l, w_l] float64: <f1[q], f2[p]> / sqrt(C), then three floor-sized
    2 x 2 means over the target dims (core/corr.py:22-28, 53-69)."""
    P, h, w, C = f1.shape
    a = np.asarray(f1, np.float64).reshape(P, h * w, C)
    b = np.asarray(f2, np.float64).reshape(P, h * w, C)
    v = (np.einsum("pic,pjc->pij", a, b) / np.sqrt(float(C))).reshape(P * h * w, h, w)
    lv = [v]
    for _ in range(3):
        lv.append(_pool(lv[-1], 1, 2))
    return lv


def feature_pyramid_ref(f2):
    """f2 [P, h, w, C] -> [f2, three floor-sized 2 x 2 means] as float64 [P, h_l, w_l, C] (AlternateCorrBlock, core/corr.py:78-82)."""
    lv = [np.asarray(f2, np.float64)]
    for _ in range(3):
        lv.append(_pool(lv[-1], 1, 2))
    return lv


# ---------------------------------------------------------------------------------------------------------------------------
# exactness conditions
# ---------------------------------------------------------------------------------------------------------------------------
def split_roundtrip(v):
    """``fp16(v) + fp16((v - hi) * 2048) / 2048`` with the kernels' float32 steps (common.h, split_halves) -> float64."""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16).astype(F32)
        lo = ((v - hi) * F32(2048)).astype(np.float16).astype(F32)
    return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def assert_exact(v, what):
    """Every finite value survives float32 and the 16-bit hi / lo split unchanged."""
    v = np.asarray(v, np.float64)
    fin = np.isfinite(v)
    v = np.where(fin, v, 0.0)
    assert np.array_equal(v.astype(F32).astype(np.float64), v), f"{what}: not a float32"
    assert np.array_equal(split_roundtrip(v), v), f"{what}: does not survive the hi / lo split"
    assert float(np.abs(v).max(initial=0.0)) <= 448.0, f"{what}: magnitude above 448"


# ---------------------------------------------------------------------------------------------------------------------------
# seeded exact inputs (the hash uses only * + % on int64, so torch evaluates it on the device to the same values)
# ---------------------------------------------------------------------------------------------------------------------------
_M31 = 2147483647


def mix(t):
    """int64 array (numpy or torch), any values 0 <= t < 2^40 -> scrambled values in [0, 2^31 - 1)."""
    t = t % _M31
    t = (t * 48271 + 11) % _M31
    t = (t * 69621 + 7) % _M31
    return (t * 16807 + 3) % _M31


def level_values(n, l, y, x, seed=0):
    """The crafted tap (y, x) of level l in query cell n's slice: integers in [-448, 448] (int64; arguments broadcast)."""
    return mix(n * 7919 + y * 104729 + x * 1299709 + (l * 15485863 + seed * 32452843 + 1)) % 897 - 448


def crafted_levels(cells, h, w, seed=0):
    """cells: int array of global cell numbers -> four float32 arrays [len(cells), h_l, w_l] of integer taps."""
    n = np.asarray(cells, np.int64)[:, None, None]
    lv = []
    for l in range(4):
        hl, wl = h >> l, w >> l
        v = level_values(n, l, np.arange(hl, dtype=np.int64)[None, :, None], np.arange(wl, dtype=np.int64)[None, None, :], seed)
        assert v.min() >= -448 and v.max() <= 448
        lv.append(v.astype(F32))
    return lv


@functools.lru_cache(maxsize=None)
def exact_features(P, h, w, C=256, seed=0):
    """(f1, f2) float32 [P, h, w, C]: f1[q] = 16 e_k(q), f2[p][c] = 64 n with integer |n| <= 7.  Computed once; read-only."""
    q = np.arange(P * h * w, dtype=np.int64)
    k = mix(q * 31 + seed * 977 + 5) % C
    f1 = np.zeros((P * h * w, C), F32)
    f1[q, k] = 16.0
    i = np.arange(P * h * w * C, dtype=np.int64)
    f2 = ((mix(i + seed * 7919 + 13) % 15 - 7) * 64).astype(F32).reshape(P * h * w, C)
    assert np.abs(f2).max() <= 448 and np.array_equal(f2 % 64, np.zeros_like(f2))
    f1, f2 = f1.reshape(P, h, w, C), f2.reshape(P, h, w, C)
    pyr = pyramid_ref(f1, f2)
    kp, f2p = k.reshape(P, h * w), f2.reshape(P, h * w, C)
    want0 = np.stack([f2p[p][:, kp[p]].T for p in range(P)])                                  # [p, q, j] = f2[p][j][k(q)]
    assert np.array_equal(pyr[0].reshape(P, h * w, h * w), want0.astype(np.float64))
    for l, t in enumerate(pyr):
        assert np.array_equal(t, np.round(t)), f"volume level {l} is not integral"
        assert_exact(t, f"volume level {l}")
    for l, t in enumerate(feature_pyramid_ref(f2)):
        assert np.array_equal(t, np.round(t)), f"feature level {l} is not integral"
        assert_exact(t, f"feature level {l}")
    f1.setflags(write=False)
    f2.setflags(write=False)
    return f1, f2


def edge_coords(P, h, w, seed=0):
    """Coordinates for P * h * w cells, every one a multiple of 1/4, as float32 [R, P * h * w, 2] (R lookups' worth).  In order:
    per level and side the first coordinate whose window is wholly outside (s = -5.25: taps -10 .. -1; s = w_l + 4) and its
    neighbour with exactly one column / row inside (s = -4.75; s = w_l + 3.75), alone and paired into the four corners; integral
    coordinates; negative fractions; the four corners of the grid; the grid itself; the rest hashed over [-48, size + 48) so that
    windows straddle every edge of every level."""
    N = P * h * w
    pts = []
    mid = lambda size, j: float((mix(np.int64(j * 131 + seed + 17)) % (4 * size)) / 4.0)      # noqa: E731
    j = 0
    for l in range(4):
        wl, hl, sc = w >> l, h >> l, float(1 << l)
        xs = [-5.25 * sc, -4.75 * sc, (wl + 4) * sc, (wl + 3.75) * sc]
        ys = [-5.25 * sc, -4.75 * sc, (hl + 4) * sc, (hl + 3.75) * sc]
        for x in xs:
            pts.append((x, mid(h, j))); j += 1
        for y in ys:
            pts.append((mid(w, j), y)); j += 1
        for x in xs:                                  # both at once: a corner of the level, one tap inside at most
            for y in ys:
                pts.append((x, y))
        pts += [((wl + 3) * sc, (hl + 3) * sc), ((wl + 4.25) * sc, -5.0 * sc), (-5.0 * sc, (hl + 4.25) * sc), (-4.0 * sc, -4.0 * sc)]
    pts += [(3.0, 2.0), (0.0, 5.0), (float(w - 2), 1.0), (-3.0, -7.0), (float(w + 2), float(h + 1)), (8.0, 8.0),       # integral
            (-0.25, -0.75), (-0.5, 2.25), (3.75, -0.25), (-7.75, -1.5), (-16.25, 3.5), (2.5, -31.75),                 # negative fractions
            (0.0, 0.0), (float(w - 1), 0.0), (0.0, float(h - 1)), (float(w - 1), float(h - 1))]                        # corners
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pts = np.concatenate([np.asarray(pts, np.float64), np.stack([xs.ravel(), ys.ravel()], 1)])                          # the grid itself
    R = -(-(len(pts) + (h * w + 1) // 2) // N)
    i = np.arange(R * N - len(pts), dtype=np.int64)
    rx = (mix(2 * i + seed * 101 + 1) % (4 * (w + 96))) / 4.0 - 48.0
    ry = (mix(2 * i + seed * 101 + 2) % (4 * (h + 96))) / 4.0 - 48.0
    pts = np.concatenate([pts, np.stack([rx, ry], 1)])
    assert np.array_equal(pts * 4, np.round(pts * 4)) and np.abs(pts).max() < 4096
    c = pts.astype(F32)
    assert np.array_equal(c.astype(np.float64), pts)
    return c.reshape(R, N, 2)


_NEXT = lambda v, to: float(np.nextafter(F32(v), F32(to)))      # noqa: E731
HOSTILE_NONFINITE = [float("nan"), float("inf"), float("-inf")]
HOSTILE_HUGE = [3e9, -3e9, 1e30, -1e30,
                1.0e6, _NEXT(1.0e6, 2e6), _NEXT(1.0e6, 0), -1.0e6, _NEXT(-1.0e6, -2e6), _NEXT(-1.0e6, 0)]      # where the clamp starts


def hostile_coords(coords):
    """coords [N, 2] -> (a copy with hostile cells scattered among the ordinary ones, rows that must be NaN, rows that must be 0).
    Every hostile value stands once in x and once in y, the cell's other coordinate stays ordinary."""
    c = np.array(coords, F32)
    N = c.shape[0]
    vals = HOSTILE_NONFINITE + HOSTILE_HUGE
    step = N // (2 * len(vals) + 1)
    assert step >= 2, "hostile cells need ordinary neighbours"
    nan_rows, zero_rows = [], []
    for i, v in enumerate(vals + vals):
        row, axis = 1 + i * step, i // len(vals)
        c[row, axis] = v
        (nan_rows if not np.isfinite(F32(v)) else zero_rows).append(row)
    return c, np.asarray(nan_rows), np.asarray(zero_rows)


@functools.lru_cache(maxsize=None)
def exact_case(P, h, w):
    """The shared crafted case of a shape: levels [N, h_l, w_l], coords [R, N, 2], expected values and mag [R, N, 324] (float64).
    Computed once; callers must not modify it."""
    N = P * h * w
    levels = crafted_levels(np.arange(N), h, w)
    coords = edge_coords(P, h, w)
    want, mag = zip(*(lookup_ref(levels, c) for c in coords))
    want, mag = np.stack(want), np.stack(mag)
    assert_exact(want, f"expected lookup at {(P, h, w)}")
    assert np.array_equal(lookup_f32(levels, coords[0]).astype(np.float64), want[0])         # another summation order, in float32
    for a in levels + [coords, want, mag]:
        a.setflags(write=False)
    return {"levels": levels, "coords": coords, "want": want, "mag": mag}
