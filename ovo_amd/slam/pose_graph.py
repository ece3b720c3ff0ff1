"""The pose graph behind `IcpTracker(close_loops=True)`: keyframe poses corrected by the loop edges `ovo_icp_align_batch`
verified.  Host code in f64 -- a few hundred 6 x 6 blocks per closure, nothing for a GPU.

    node k     X_k, 4 x 4: keyframe camera k -> the first camera.  X_0 is fixed.
    edge       (i, j, Z, W): Z is what an alignment with reference i and current j returns (camera j -> camera i), W its 6 x 6 J^T J
               (`icp_utils.information`).  Error e = log(X_i^-1 X_j Z^-1), a twist with the rotation first; cost = sum e^T W e.
    update     X_k <- exp(d_k) X_k (a LEFT perturbation, the one the alignment's J is taken in: W needs no change of frame).

With E = X_i^-1 X_j Z^-1:  X_j <- exp(d) X_j gives E <- exp(Ad(X_i^-1) d) E, and X_i <- exp(d) X_i gives E <- exp(-Ad(X_i^-1) d) E, so
de/dd_j = Jl^-1(e) Ad(X_i^-1) = -de/dd_i, with Jl^-1(e) = sum_n B_n / n! ad(e)^n (Bernoulli numbers; carried to ad^6: the next term is
e^8 / 1 209 600, below f64 for any residual under 0.1)."""
from __future__ import annotations

from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from ..utils.icp_utils import rigid_inverse, se3_exp, se3_log

Edge = Tuple[int, int, np.ndarray, np.ndarray]
DENSE_NODES = 300                                          # above it the normal equations go through scipy.sparse
MAX_STEPS, STEP_TOL = 50, 1e-12


def _hat(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def adjoint(X) -> np.ndarray:
    """Ad(X) for twists (rotation | translation): exp(Ad(X) d) = X exp(d) X^-1."""
    R, t = X[:3, :3], X[:3, 3]
    out = np.zeros((6, 6))
    out[:3, :3] = out[3:, 3:] = R
    out[3:, :3] = _hat(t) @ R
    return out


def left_jacobian_inverse(e) -> np.ndarray:
    """Jl^-1(e): log(exp(d) exp(e)) = e + Jl^-1(e) d + O(d^2)."""
    ad = np.zeros((6, 6))
    ad[:3, :3] = ad[3:, 3:] = _hat(e[:3])
    ad[3:, :3] = _hat(e[3:])
    ad2 = ad @ ad
    ad4 = ad2 @ ad2
    return np.eye(6) - 0.5 * ad + ad2 / 12.0 - ad4 / 720.0 + (ad4 @ ad2) / 30240.0


def edge_error(Xi, Xj, Z) -> np.ndarray:
    return se3_log(rigid_inverse(Xi) @ Xj @ rigid_inverse(Z))


def cost(X: Sequence[np.ndarray], edges: Sequence[Edge]) -> float:
    total = 0.0
    for i, j, Z, W in edges:
        e = edge_error(X[i], X[j], Z)
        total += float(e @ W @ e)
    return total


def _normal_equations(X, edges, n):
    """(blocks {(a, b): 6 x 6, a <= b over the free nodes 1 .. n - 1}, gradient f64[6 (n - 1)])."""
    blocks: Dict[Tuple[int, int], np.ndarray] = {}
    g = np.zeros(6 * (n - 1))
    for i, j, Z, W in edges:
        e = edge_error(X[i], X[j], Z)
        Jj = left_jacobian_inverse(e) @ adjoint(rigid_inverse(X[i]))
        JW = Jj.T @ W
        H, b = JW @ Jj, JW @ e
        for a, sa in ((i, -1.0), (j, 1.0)):
            if a == 0:
                continue
            g[6 * (a - 1):6 * a] += sa * b
            for c, sc in ((i, -1.0), (j, 1.0)):
                if c == 0 or c < a:
                    continue
                key = (a, c)
                blocks[key] = blocks.get(key, 0.0) + (sa * sc) * H
    return blocks, g


def _solve(blocks, g, n, lam):
    free = n - 1
    if n <= DENSE_NODES:
        H = np.zeros((6 * free, 6 * free))
        for (a, c), B in blocks.items():
            H[6 * (a - 1):6 * a, 6 * (c - 1):6 * c] += B
            if a != c:
                H[6 * (c - 1):6 * c, 6 * (a - 1):6 * a] += B.T
        H[np.diag_indices_from(H)] += lam * H.diagonal()
        return np.linalg.solve(H, -g)
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    rows, cols, vals = [], [], []
    r6, c6 = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
    for (a, c), B in blocks.items():
        if a == c:
            B = B + lam * np.diag(B.diagonal())
        rows.append(6 * (a - 1) + r6); cols.append(6 * (c - 1) + c6); vals.append(B.reshape(-1))
        if a != c:
            rows.append(6 * (c - 1) + c6); cols.append(6 * (a - 1) + r6); vals.append(B.reshape(-1))
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * free, 6 * free))
    return spsolve(H, -g)


def optimise(poses: Sequence[np.ndarray], edges: Sequence[Edge]) -> Tuple[List[np.ndarray], Dict[str, Any]]:
    """Gauss-Newton with Levenberg damping (only raised when a step does not lower the cost) over the nodes 1 .. n - 1.  Stops at
    max |d| < 1e-12 or after 50 steps.  Returns (poses, {"cost0", "cost", "steps", "improved"}); a result whose cost is not below the start cost is
    discarded: the start poses come back as they were given ("improved" False).  Every free node must be reached by an edge."""
    X0 = [np.array(p, dtype=np.float64) for p in poses]
    n = len(X0)
    edges = [(int(i), int(j), np.asarray(Z, dtype=np.float64), np.asarray(W, dtype=np.float64)) for i, j, Z, W in edges]
    if any(not (0 <= i < n and 0 <= j < n and i != j) for i, j, _, _ in edges):
        raise ValueError("pose graph: an edge names a node that does not exist, or one node twice")
    c0 = cost(X0, edges)
    info = {"cost0": c0, "cost": c0, "steps": 0, "improved": False}
    if n < 2 or not edges:
        return X0, info
    X, c, lam = X0, c0, 0.0
    for step in range(MAX_STEPS):
        blocks, g = _normal_equations(X, edges, n)
        done = False
        while True:
            try:
                d = _solve(blocks, g, n, lam)
            except np.linalg.LinAlgError:                  # singular normal equations (a node no weighted edge reaches): no step
                d = np.full(6 * (n - 1), np.nan)
            trial = [X[0]] + [se3_exp(d[6 * (k - 1):6 * k]) @ X[k] for k in range(1, n)]
            ct = cost(trial, edges)
            small = not np.abs(d).max() >= STEP_TOL       # (a NaN step ends the iteration too)
            if ct < c or (small and ct <= c):
                X, c, lam = trial, ct, lam * 0.1 if lam > 1e-9 else 0.0
                done = small
                break
            if small or lam > 1e9:
                done = True
                break
            lam = max(10.0 * lam, 1e-6)
        info["steps"] = step + 1
        if done:
            break
    if not c < c0:
        return X0, info
    info.update(cost=c, improved=True)
    return X, info
