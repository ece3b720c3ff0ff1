"""The contract of ovo_tsdf_mesh_normals / ovo_tsdf_raycast_normals and of tsdf_utils.shade_normals (include/ovo_hip.h) restated in
numpy on top of tsdf_restatement (T), mesh_restatement (M) and tsdf_color_restatement (TC), written from the contract's text and not from the HIP code.

Two switches, as in tsdf_restatement: `np.float64` -- THE REFERENCE -- and `np.float32`, every operation one numpy operation of that type.  What is f32
in both forms because the contract states it in f32: the volume, the descriptors, a mesh vertex's t ("emit's own bits").  The largest distance
between the two forms on the same inputs, "d32n", is the size of legitimate rounding differences."""
import numpy as np

import mesh_restatement as M
import tsdf_color_restatement as TC
import tsdf_restatement as T

BOTH, HI, LO, NONE = 0, 1, 2, 3                            # the branch an axis of a gradient took


def _neighbours(vol, obs, idx, a):
    """(lo_ok, hi_ok, F(m), F(r)) along axis a for the voxels idx [N, 3] (x, y, z); F of a neighbour that fails its index test is never looked at."""
    nz, ny, nx = vol.shape[:3]
    n = (nx, ny, nz)
    m, r = idx.copy(), idx.copy()
    m[:, a] -= 1
    r[:, a] += 1
    lo_in, hi_in = idx[:, a] >= 1, idx[:, a] <= n[a] - 2
    m[:, a], r[:, a] = np.where(lo_in, m[:, a], idx[:, a]), np.where(hi_in, r[:, a], idx[:, a])
    at = lambda p: (p[:, 2], p[:, 1], p[:, 0])
    return lo_in & obs[at(m)], hi_in & obs[at(r)], vol[at(m) + (0,)], vol[at(r) + (0,)]


def gradient(vol, obs, idx, dtype=np.float64):
    """grad(p; obs) [N, 3] of `dtype` for the voxels idx [N, 3] (x, y, z) of vol [nz, ny, nx, 2]; obs: bool [nz, ny, nx] over the WHOLE volume."""
    vol, idx = np.asarray(vol), np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    Fp = vol[idx[:, 2], idx[:, 1], idx[:, 0], 0].astype(dtype)
    g = np.zeros((len(idx), 3), dtype=dtype)
    for a in range(3):
        lo_ok, hi_ok, Fm, Fr = _neighbours(vol, obs, idx, a)
        Fm, Fr = Fm.astype(dtype), Fr.astype(dtype)
        with np.errstate(invalid="ignore"):
            g[:, a] = np.where(lo_ok & hi_ok, (Fr - Fm) * dtype(0.5), np.where(hi_ok, Fr - Fp, np.where(lo_ok, Fp - Fm, dtype(0))))
    return g


def branches(vol, obs, idx):
    """[N, 3] of BOTH / HI / LO / NONE: the case each axis of gradient(vol, obs, idx) took."""
    vol, idx = np.asarray(vol), np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    out = np.zeros((len(idx), 3), dtype=np.int64)
    for a in range(3):
        lo_ok, hi_ok, _, _ = _neighbours(vol, obs, idx, a)
        out[:, a] = np.where(lo_ok & hi_ok, BOTH, np.where(hi_ok, HI, np.where(lo_ok, LO, NONE)))
    return out


def length(g):
    """sqrt(g0 g0 + g1 g1 + g2 g2): products first, then the two sums left to right, in g's type."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])


def unit(g):
    """g / length where the length is positive and finite, three +0.0 elsewhere."""
    ln = length(g)
    with np.errstate(invalid="ignore"):
        ok = (ln > 0) & np.isfinite(ln)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok[..., None], g / np.where(ok, ln, 1)[..., None], np.zeros_like(g))


def lerp(p, q, t):
    return p + t * (q - p)


def mesh_normals(vol, sp, box=None, min_weight=1.0, dtype=np.float64):
    """(normals [V, 3] of `dtype` in emit order, details): unit(lerp(grad(p), grad(q), t)) with obs = OBSERVED over the whole volume and the f32 t of
    the vertex.  details: "p", "q", "t" (TC.mesh_edges), "g" the blended gradient before normalisation, "branches" [V, 2, 3] of both ends."""
    vol = np.asarray(vol, dtype=np.float32)
    p, q, t = TC.mesh_edges(vol, sp, box, min_weight)
    obs = M.observed(vol, min_weight)
    gp, gq = gradient(vol, obs, p, dtype), gradient(vol, obs, q, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        g = lerp(gp, gq, t.astype(dtype)[:, None])
    return unit(g), {"p": p, "q": q, "t": t, "g": g, "branches": np.stack([branches(vol, obs, p), branches(vol, obs, q)], 1)}


def raycast_normals(vol, sp, cam, dz, dtype=np.float64, knife_edges=True):
    """(normals [h, w, 3] of `dtype`, details) on top of T.raycast: its "hit", "knife" and "steps" say where and at which sample k = steps - 1 a pixel
    hit.  The samples k - 1 and k are formed again by the march's own expressions; each gradient component is the trilinear blend (x, then y, then
    z) of grad(corner; W > 0) over the sample's eight corners; g = lerp(g_{k-1}, g_k, s) with the depth's s; the pixel is unit(g).
    details: T.raycast's, and "depth" (T.raycast's), "depth_again" (from the samples formed here: the same bits), "k", "g" [h, w, 3] before
    normalisation, "branches" [N, 2, 8, 3] of the hit pixels in row-major order."""
    depth, det = T.raycast(vol, sp, cam, dz, dtype, knife_edges=knife_edges)
    vol = np.asarray(vol)
    h, w = cam["h"], cam["w"]
    hit = det["hit"]
    pv, pu = np.nonzero(hit)
    k = det["steps"][hit] - 1
    seen = vol[..., 1] > 0
    fx, fy, cx, cy = (dtype(cam[x]) for x in ("fx", "fy", "cx", "cy"))
    near, dzt = dtype(cam["near"]), dtype(np.float32(dz))
    voxel, org = dtype(sp["voxel"]), sp["origin"].astype(dtype)
    c = cam["c2w"].astype(dtype)
    dcx, dcy = (pu.astype(dtype) - cx) / fx, (pv.astype(dtype) - cy) / fy
    dw = [(c[r, 0] * dcx + c[r, 1] * dcy) + c[r, 2] * dtype(1) for r in range(3)]
    F = vol[..., 0].astype(dtype)
    fs, gs, br = [], [], []
    for e in (0, 1):
        zk = near + (k - 1 + e).astype(dtype) * dzt
        gc = [((c[a, 3] + zk * dw[a]) - org[a]) / voxel for a in range(3)]
        bf = [np.floor(x) for x in gc]
        t = [x - y for x, y in zip(gc, bf)]
        b = np.stack([y.astype(np.int64) for y in bf], 1)                                       # valid samples: within [0, n - 2]
        corner = [b + np.array([cn & 1, cn >> 1 & 1, cn >> 2]) for cn in range(8)]
        blend = lambda v: lerp(lerp(lerp(v[0], v[1], t[0]), lerp(v[2], v[3], t[0]), t[1]), lerp(lerp(v[4], v[5], t[0]), lerp(v[6], v[7], t[0]), t[1]), t[2])
        fs.append(blend([F[p[:, 2], p[:, 1], p[:, 0]] for p in corner]))
        grads = [gradient(vol, seen, p, dtype) for p in corner]
        gs.append(np.stack([blend([gr[:, a] for gr in grads]) for a in range(3)], 1))
        br.append(np.stack([branches(vol, seen, p) for p in corner], 1))
        assert all(seen[p[:, 2], p[:, 1], p[:, 0]].all() for p in corner)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = fs[0] / (fs[0] - fs[1])
        g_hit = lerp(gs[0], gs[1], s[:, None])
        z_hit = (near + (k - 1).astype(dtype) * dzt) + dzt * s
    g = np.zeros((h, w, 3), dtype=dtype)
    g[hit] = g_hit
    again = np.zeros((h, w), dtype=dtype)
    again[hit] = z_hit
    kk = np.full((h, w), -1, dtype=np.int64)
    kk[hit] = k
    out = dict(det)
    out.update(depth=depth, depth_again=again, k=kk, g=g, branches=np.stack(br, 1) if len(k) else np.zeros((0, 2, 8, 3), dtype=np.int64))
    return unit(g), out


def rays(K, c2w, h, w, dtype=np.float64):
    """The unit ray of every pixel in the frame c2w maps to: [h, w, 3]."""
    K, c = np.asarray(K, dtype=np.float32).astype(dtype), np.asarray(c2w, dtype=np.float32).astype(dtype)
    u, v = np.meshgrid((np.arange(w).astype(dtype) - K[0, 2]) / K[0, 0], (np.arange(h).astype(dtype) - K[1, 2]) / K[1, 1])
    d = np.stack([u, v, np.ones_like(u)], -1) @ c[:3, :3].T
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def shade(normals, K, c2w, rgb=None, ambient=0.2, dtype=np.float64):
    """(u8 [h, w, 3], the value before rint): i = ambient + (1 - ambient) clamp(-n . d, 0, 1); 255 i, or i * rgb; (0, 0, 0) where the normal is zero."""
    n = np.asarray(normals).astype(dtype)
    h, w = n.shape[:2]
    i = dtype(ambient) + (dtype(1) - dtype(ambient)) * np.clip(-(n * rays(K, c2w, h, w, dtype)).sum(-1), 0, 1)
    base = np.full((h, w, 3), 255, dtype=dtype) if rgb is None else np.asarray(rgb).astype(dtype)
    pre = np.where((n != 0).any(-1, keepdims=True), i[..., None] * base, 0)
    return np.rint(pre).astype(np.uint8), pre
