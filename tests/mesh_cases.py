"""Volumes for the mesh tests (test_mesh_host.py on the CPU, test_gpu_mesh.py on the GPU): each is (sp, vol f32[nz, ny, nx, 2], box or None, min_weight).
Analytic signed distances are evaluated in f64 at the voxel positions origin + voxel * index of the f32 descriptor and rounded to f32 once."""
import numpy as np

import tsdf_restatement as T

SQRT3 = float(np.sqrt(3.0))


def grid(sp):
    """f64 positions Z, Y, X [nz, ny, nx] of the voxels of sp: origin + voxel * index with the f32 descriptor's values, no rounding."""
    ax = [float(sp["origin"][a]) + float(sp["voxel"]) * np.arange(sp["dims"][a], dtype=np.float64) for a in range(3)]
    return np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")


def from_sdf(sp, sdf, weight=1.0):
    """F = clip(sdf / trunc, -1, 1) rounded to f32, every voxel with the weight given (an array or a number)."""
    vol = T.empty(sp, np.float32)
    vol[..., 0] = np.clip(sdf / float(sp["trunc"]), -1.0, 1.0)
    vol[..., 1] = weight
    return vol


SPHERE = dict(center=(1.2307, 1.1713, 1.2109), r=0.8)       # off the grid in every coordinate, 3 voxels and more from every face of the volume
TORUS = dict(center=(1.1871, 1.2203, 1.1609), R=0.7, r=0.3)


def solid_spec():
    return T.spec((24, 24, 24), 0.1, (0.013, -0.021, 0.007), 0.35)      # trunc 0.35 >= 2 sqrt(3) voxel = 0.3464...


def sphere_sdf(sp):
    Z, Y, X = grid(sp)
    c = SPHERE["center"]
    return np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - SPHERE["r"]


def sphere_case():
    sp = solid_spec()
    return sp, from_sdf(sp, sphere_sdf(sp)), None, 1.0


def torus_case():
    sp = solid_spec()
    Z, Y, X = grid(sp)
    c = TORUS["center"]
    ring = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - TORUS["R"]
    return sp, from_sdf(sp, np.sqrt(ring ** 2 + (Z - c[2]) ** 2) - TORUS["r"]), None, 1.0


def plane_case(dims, voxel=0.11, origin=(-1.69, -0.91, 0.66), trunc=0.4, normal=(0.31, -0.52, 1.0), through=0.45):
    """A tilted plane through the point at the fraction `through` of the volume's diagonal: it crosses every row of a long thin volume."""
    sp = T.spec(dims, voxel, origin, trunc)
    Z, Y, X = grid(sp)
    n = np.asarray(normal, dtype=np.float64) / np.linalg.norm(normal)
    at = np.asarray([float(o) for o in sp["origin"]]) + through * float(sp["voxel"]) * (np.asarray(dims) - 1)
    return sp, from_sdf(sp, n[0] * (X - at[0]) + n[1] * (Y - at[1]) + n[2] * (Z - at[2])), None, 1.0


def long_plane_case(dims):
    """130 x 9 x 7, 300 x 5 x 4: the plane runs along x and falls by 0.8 of the volume's height over its length, so that it meets rows from the
    first voxel of a row to the last."""
    return plane_case(dims, normal=(0.8 * (dims[2] - 1) / (dims[0] - 1), 0.6, 1.0), through=0.5)


def holes_case(min_weight=1.0):
    """33 x 17 x 9 with a tilted plane; weights 0 .. 3 at random: about 30 % of the voxels have weight 0; with min_weight 2 about 40 % are unobserved."""
    sp, vol, _, _ = plane_case((33, 17, 9))
    rng = np.random.default_rng(11)
    vol[..., 1] = rng.choice([0.0, 1.0, 2.0, 3.0], size=vol.shape[:3], p=[0.3, 0.1, 0.3, 0.3]).astype(np.float32)
    return sp, vol, None, float(min_weight)


def specials_case():
    """A plane volume into which the values the contract names are written: F == 0, -0.0, 1, -1, NaN, |F| > 1 with positive weight, a NaN weight."""
    sp, vol, _, _ = plane_case((9, 8, 7), normal=(0.3, 0.2, 1.0))
    # (z, y, x) near the plane z ~ 2.7 voxels: every special value sits on a corner of cells the surface passes through
    for (z, y, x), f in zip(((2, 2, 2), (3, 3, 3), (2, 4, 5), (3, 5, 2), (2, 5, 6), (3, 2, 6), (2, 6, 3), (3, 6, 6)),
                            (0.0, -0.0, 1.0, -1.0, np.nan, 1.5, 0.0, -0.0)):
        vol[z, y, x, 0] = f
    vol[4, 4, 4, 1] = np.nan
    return sp, vol, None, 1.0


def box_case():
    """A box with odd lo and even hi inside a larger volume."""
    sp, vol, _, _ = plane_case((21, 14, 12), normal=(0.31, -0.52, 1.0))
    return sp, vol, ((3, 1, 1), (18, 12, 10)), 1.0


def single_cell_case(mask):
    """2 x 2 x 2: corner c = x + 2 y + 4 z is inside iff bit c of mask; magnitudes differ from corner to corner."""
    sp = T.spec((2, 2, 2), 0.25, (0.4, -0.3, 1.1), 0.8)
    vol = T.empty(sp, np.float32)
    for c in range(8):
        mag = np.float32(0.11 + 0.09 * c)
        vol[c >> 2, (c >> 1) & 1, c & 1] = (-mag if (mask >> c) & 1 else mag, 1.0)
    return sp, vol, None, 1.0


# a lone corner, a face, an edge pair, a diagonal pair, a complement: among them every tetrahedron meets a two-against-two mask
# (test_mesh_host.test_single_cell_masks_reach_every_quad checks that from the table)
SINGLE_CELL_MASKS = (0x01, 0x80, 0x0F, 0x33, 0x55, 0x81, 0x69, 0x96, 0x17, 0xFE)
