"""`ovo_render_points` restated on the CPU (include/ovo_hip.h has the contract): the reference of tests/test_gpu_render.py.

(u, v) come from `oracle.geometry.project`, which the geometry tests pin bit for bit to the GPU's `project()`.  zc -- the un-normalised camera z,
a four-term chain of one product and three fused multiply-adds -- is restated with exact rational arithmetic: every step is evaluated in
`fractions.Fraction` and rounded ONCE to the nearest f32, ties to even, which is what `__fmul_rn` / `__fmaf_rn` do.  Plain numpy f32 is not that
function (it rounds the product before the sum).  Then a brute-force minimum of the 64-bit keys float_bits(zc) << 32 | row per pixel.

Two flavours:
  render(...)          any finite scene, a Python loop per point and covered pixel: a few thousand points
  render_lattice(...)  vectorised, for LATTICE scenes -- coordinates multiples of 1/64 in [-8, 8], w2c a signed axis permutation with a dyadic
                       translation -- where every product and sum of the chain is exact, so plain numpy f32 IS the chain (asserted against an f64
                       evaluation); the minimum is `np.minimum.at` on uint64
Both return (row i32[h,w], depth f32[h,w], count i32[h,w]): count = number of covering points per pixel."""
from fractions import Fraction

import numpy as np

from oracle import geometry as OG

INT_MIN = -2 ** 31
KEY_EMPTY = np.uint64(2 ** 64 - 1)


def round_f32(q: Fraction) -> np.float32:
    """The f32 nearest to the rational q, ties to even; overflow to +-inf, gradual underflow (IEEE 754 binary32)."""
    if q == 0:
        return np.float32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()        # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                        # 2^e <= a < 2^(e+1)
    e = max(e, -126)                                                  # subnormals share the smallest normal's spacing
    ulp = Fraction(2) ** (e - 23)
    m, rem = divmod(a, ulp)
    m = int(m)
    if 2 * rem > ulp or (2 * rem == ulp and m & 1):
        m += 1
    if m * ulp >= Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * float(m * ulp))                          # (m * ulp is an f32: the conversion through f64 is exact)


def chain4(m, x, y, z, w=1.0) -> np.float32:
    """dot4 of csrc/projection.h: fl(fl(fl(fl(m0 x) + m1 y) + m2 z) + m3 w), every fl one rounding of the exact value."""
    a = round_f32(Fraction(float(m[0])) * Fraction(float(x)))
    for mk, c in ((m[1], y), (m[2], z), (m[3], w)):
        a = round_f32(Fraction(float(mk)) * Fraction(float(c)) + Fraction(float(a)))
    return a


def depths(xyz: np.ndarray, w2c: np.ndarray, uv: np.ndarray) -> np.ndarray:
    """zc f32[n] by the exact chain.  A row with a non-finite coordinate has no rational value; its zc is reported as NaN, which is allowed only
    because such a row never contributes whatever its zc: its pixel must already be INT_MIN (asserted)."""
    w2c = np.asarray(w2c, np.float32).reshape(4, 4)
    zc = np.empty(xyz.shape[0], np.float32)
    for i, p in enumerate(xyz):
        if np.isfinite(p).all():
            zc[i] = chain4(w2c[2], p[0], p[1], p[2])
        else:
            assert uv[i, 0] == INT_MIN or uv[i, 1] == INT_MIN, f"row {i} is not finite and still has a pixel"
            zc[i] = np.nan
    return zc


def contributes(zc, uv, h, w, radius, near, far):
    u, v = uv[:, 0].astype(np.int64), uv[:, 1].astype(np.int64)
    with np.errstate(invalid="ignore"):
        return (zc >= np.float32(near)) & (zc <= np.float32(far)) & (u >= -radius) & (u < w + radius) & (v >= -radius) & (v < h + radius)


def keys_of(zc: np.ndarray) -> np.ndarray:
    return (zc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(zc.shape[0], dtype=np.uint64)


def decode(keys: np.ndarray):
    hit = keys != KEY_EMPTY
    row = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(np.float32)
    return row, depth


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def render(xyz, w2c, K, h, w, radius, near, far, zc=None):
    """The brute-force reference.  `zc`: depths computed earlier for the same xyz and w2c (they do not depend on the radius)."""
    xyz = _f32(xyz).reshape(-1, 3)
    uv = OG.project(xyz, _f32(K), _f32(w2c)) if xyz.shape[0] else np.zeros((0, 2), np.int32)
    zc = depths(xyz, w2c, uv) if zc is None else zc
    ok = contributes(zc, uv, h, w, radius, near, far)
    key = keys_of(zc)
    keys = np.full((h, w), KEY_EMPTY, np.uint64)
    count = np.zeros((h, w), np.int32)
    for i in np.nonzero(ok)[0]:
        u, v = int(uv[i, 0]), int(uv[i, 1])
        for y in range(max(v - radius, 0), min(v + radius, h - 1) + 1):
            for x in range(max(u - radius, 0), min(u + radius, w - 1) + 1):
                count[y, x] += 1
                if key[i] < keys[y, x]:
                    keys[y, x] = key[i]
    return decode(keys) + (count,)


def lattice_depths(xyz, w2c) -> np.ndarray:
    """zc of a lattice scene in plain numpy f32, asserted exact: the f64 evaluation of the same products and sums has the same value."""
    xyz, w2c = _f32(xyz), _f32(w2c).reshape(4, 4)
    m = w2c[2]
    z32 = ((m[0] * xyz[:, 0] + m[1] * xyz[:, 1]) + m[2] * xyz[:, 2]) + m[3]
    m64, p64 = m.astype(np.float64), xyz.astype(np.float64)
    z64 = ((m64[0] * p64[:, 0] + m64[1] * p64[:, 1]) + m64[2] * p64[:, 2]) + m64[3]
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64), "not a lattice scene: a step of the chain rounds"
    return z32


def render_lattice(xyz, w2c, K, h, w, radius, near, far):
    xyz = _f32(xyz).reshape(-1, 3)
    uv = OG.project(xyz, _f32(K), _f32(w2c))
    zc = lattice_depths(xyz, w2c)
    ok = contributes(zc, uv, h, w, radius, near, far)
    key = keys_of(zc)[ok]
    u, v = uv[ok, 0].astype(np.int64), uv[ok, 1].astype(np.int64)
    keys = np.full(h * w, KEY_EMPTY, np.uint64)
    count = np.zeros(h * w, np.int32)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = u + dx, v + dy
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            px = y[inside] * w + x[inside]
            np.minimum.at(keys, px, key[inside])
            np.add.at(count, px, 1)
    row, depth = decode(keys.reshape(h, w))
    return row, depth, count.reshape(h, w)


# ---------------------------------------------------------------------------------------------------- scenes
K_SMALL = np.array([[60, 0, 31.5], [0, 60, 23.5], [0, 0, 1]], np.float32)


def rot(axis: int, a: float) -> np.ndarray:
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def general_pose() -> np.ndarray:
    """c2w f32[4,4]: three composed rotations (0.2, -0.3, 0.1 rad about x, y, z) and a translation."""
    m = rot(0, 0.2) @ rot(1, -0.3) @ rot(2, 0.1)
    m[:3, 3] = (0.4, -0.25, 0.3)
    return m.astype(np.float32)


def general_scene(n: int = 6000, seed: int = 11):
    """(xyz f32[n,3] in the world, c2w): points generated in the camera frame of `general_pose` and moved to the world.  x uniform in +-1.6, y in
    +-1.2, z = 1.5 or 2.5 with equal chance + N(0, 0.02); the first 200 with z uniform in [-1, 0.05] (behind or at the camera); rows 200-259 exact
    copies of rows 260-319 (ties broken by row)."""
    rng = np.random.default_rng(seed)
    cam = np.empty((n, 3))
    cam[:, 0] = rng.uniform(-1.6, 1.6, n)
    cam[:, 1] = rng.uniform(-1.2, 1.2, n)
    cam[:, 2] = np.where(rng.random(n) < 0.5, 1.5, 2.5) + rng.normal(0.0, 0.02, n)
    k = min(200, n)
    cam[:k, 2] = rng.uniform(-1.0, 0.05, k)
    c2w = general_pose()
    xyz = (cam @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3].astype(np.float64)).astype(np.float32)
    if n >= 320:
        xyz[200:260] = xyz[260:320]
    return xyz, c2w


def lattice_scene(n: int, seed: int = 5):
    """(xyz f32[n,3], w2c f32[4,4]): coordinates multiples of 1/64, x in [-8, 8], y and z in [-3, 3] (a corridor in front of the camera, so that
    most of it is in view); the camera looks along world +x from x = -9.5 (camera z = x + 9.5, camera x = -z + 0.25, camera y = y - 0.5): a
    signed axis permutation with a dyadic translation."""
    rng = np.random.default_rng(seed)
    xyz = (np.concatenate([rng.integers(-512, 513, (n, 1)), rng.integers(-192, 193, (n, 2))], axis=1) / 64.0).astype(np.float32)
    w2c = np.array([[0, 0, -1, 0.25], [0, 1, 0, -0.5], [1, 0, 0, 9.5], [0, 0, 0, 1]], np.float32)
    return xyz, w2c
