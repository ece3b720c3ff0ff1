"""Loop closing in IcpTracker restated in plain numpy, written from the contract's text: the SE(3) logarithm, the pose
graph's cost, candidate selection, the acceptance rule, and `LoopTracker` -- icp_restatement's Tracker with close_loops, in its f64 and f32 forms
(the alignment's per-pixel arithmetic switches; the graph is f64 in both, as the contract states it).

The graph's minimum is NOT restated as a second Gauss-Newton: `minimise` hands the residuals to scipy.optimize.least_squares (numerical
Jacobian, its own trust region), a different road to the minimum of the same f64 function."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402


def se3_log(T):
    """(rotation | translation) with se3_exp(se3_log(T)) = T, for angles below pi."""
    T = np.asarray(T, dtype=np.float64)
    Rm, t = T[:3, :3], T[:3, 3]
    v = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]]) / 2
    s, c = np.linalg.norm(v), (np.trace(Rm) - 1) / 2
    th = math.atan2(s, c)
    w = v * (th / s) if th >= 1e-4 else v * (1 + th * th / 6)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if th >= 1e-4:
        b, cc = (1 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    else:
        b, cc = 0.5 - th * th / 24, 1 / 6 - th * th / 120
    V = np.eye(3) + b * k + cc * (k @ k)
    return np.concatenate([w, np.linalg.solve(V, t)])


def inv(T):
    return np.linalg.inv(np.asarray(T, dtype=np.float64))


def residuals(X, edges):
    """One 6-vector per edge, whitened: |residuals|^2 is the cost.  W = U^T U by Cholesky (W must be positive definite)."""
    out = []
    for i, j, Z, W in edges:
        e = se3_log(inv(X[i]) @ X[j] @ inv(Z))
        out.append(np.linalg.cholesky(W).T @ e)
    return np.concatenate(out)


def cost(X, edges):
    total = 0.0
    for i, j, Z, W in edges:
        e = se3_log(inv(X[i]) @ X[j] @ inv(Z))
        total += float(e @ W @ e)
    return total


def minimise(X0, edges):
    """The minimum over X_1 .. X_{n-1} by scipy.optimize.least_squares, parametrised as X_k = exp(p_k) X0_k.  Returns (poses, cost)."""
    from scipy.optimize import least_squares
    n = len(X0)

    def poses(p):
        return [np.asarray(X0[0], np.float64)] + [R.se3_exp(p[6 * (k - 1):6 * k]) @ X0[k] for k in range(1, n)]

    sol = least_squares(lambda p: residuals(poses(p), edges), np.zeros(6 * (n - 1)), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0)
    X = poses(sol.x)
    return X, cost(X, edges)


def offset(T):
    return R.pose_distance(np.eye(4), T)


def select_candidates(X, n, available, min_gap, radius, angle_deg, max_candidates):
    """[(k, G_k)]: available k <= n - min_gap with G_k = X_k^-1 X_n inside radius and angle; the max_candidates of smallest translation, ties to the lower k."""
    rows = []
    for k in sorted(available):
        if k <= n - min_gap:
            G = inv(X[k]) @ X[n]
            t, a = offset(G)
            if t <= radius and a <= angle_deg:
                rows.append((t, k, G))
    rows = sorted(rows, key=lambda r: (r[0], r[1]))[:max_candidates]
    return [(k, G) for _, k, G in rows]


def accept(res, G, pixels, min_overlap, max_rms, max_correction):
    if res["state"] != R.OK or res["pairs"] < min_overlap * pixels or not res["rms"] <= max_rms:
        return False
    t, a = R.pose_distance(G, res["T"])
    return t <= max_correction[0] and a <= max_correction[1]


def information(sums):
    W = np.zeros((6, 6))
    for e, (i, j) in enumerate(R.IU):
        W[i, j] = W[j, i] = sums[e]
    return W


class LoopTracker(R.Tracker):
    """R.Tracker with the six steps of close_loops on every new keyframe.  Records per frame: `big_change`; per closure attempt: `attempts`
    (n, candidates, accepted, applied); `edges_accepted` [(k, n)]; `kf_history`: the keyframe rows as they stood after each frame; `plain_rows`: the rows the same alignments give WITHOUT loop closing (the
    alignments are relative to the keyframe, so they do not depend on the corrections); `alignments`: how many alignments stand behind each pose."""

    def __init__(self, K, loop_min_gap=10, loop_radius=0.5, loop_angle_deg=30.0, loop_max_candidates=8, loop_iters=None, loop_dist_th=0.2,
                 loop_min_overlap=0.3, loop_max_rms=0.02, loop_max_correction=(0.3, 10.0), loop_min_shift=(0.01, 0.2), loop_max_keyframes=256,
                 solver=None, **kw):
        super().__init__(K, **kw)
        self.lp = dict(gap=loop_min_gap, radius=loop_radius, angle=loop_angle_deg, cap=loop_max_candidates, iters=loop_iters or self.iters,
                       dist_th=loop_dist_th, overlap=loop_min_overlap, rms=loop_max_rms, corr=loop_max_correction, shift=loop_min_shift,
                       keep=loop_max_keyframes)
        self.solver = solver                               # (poses, edges) -> (poses, improved): the graph optimiser under test, or None = `minimise`
        self.X, self.edges, self.db = [np.eye(4)], [], {}
        self.big, self.big_change, self.attempts, self.edges_accepted = 0, [], [], []
        self.plain_kf_c2w, self.plain_rows = np.eye(4, dtype=np.float32), []
        self.alignments, self._n_align, self.kf_history = [], 0, []

    def process(self, depth, t):
        self._process(depth, t)
        self.kf_history.append(list(self.keyframes))

    def _process(self, depth, t):
        """R.Tracker.process (whose alignment result is local to it) with the closure step on a new keyframe."""
        cur = R.prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
        row = lambda c2w: np.concatenate([np.asarray([t], np.float32), c2w[:3].reshape(12).astype(np.float32)])
        if self.kf is None:
            self.kf = cur
            self.rows.append(row(self.c2w)); self.flags.append(True); self.states.append(R.OK); self.keyframes.append(self.rows[-1])
            self.aligned_since_kf.append(0); self.plain_rows.append(self.rows[-1]); self.big_change.append(0); self.alignments.append(0)
            return
        pixels = depth.shape[0] * depth.shape[1]
        res = R.align(self.kf, cur, self.T, self.iters, self.dist_th, self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)),
                      self.min_pivot_ratio, self.dtype)
        if res["state"] != R.OK:
            self.rows.append(self.rows[-1]); self.flags.append(False); self.states.append(R.LOST); self.aligned_since_kf.append(self._since)
            self.plain_rows.append(self.plain_rows[-1]); self.big_change.append(self.big); self.alignments.append(self._n_align)
            return
        self.T = res["T"]
        self._since += 1
        self._n_align += 1
        self.c2w = (self.kf_c2w @ self.T).astype(np.float32)
        plain = (self.plain_kf_c2w @ self.T).astype(np.float32)
        self.rows.append(row(self.c2w)); self.states.append(R.OK); self.aligned_since_kf.append(self._since); self.plain_rows.append(row(plain))
        if R.keyframe_decision(self.T, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap):
            old_kf = self.kf
            self.kf, self.kf_c2w, self.T, self._since, self.plain_kf_c2w = cur, self.c2w, np.eye(4, dtype=np.float32), 0, plain
            self.flags.append(True); self.keyframes.append(self.rows[-1])
            self._close(old_kf, res, pixels)
        else:
            self.flags.append(False)
        self.big_change.append(self.big)
        self.alignments.append(self._n_align)

    def _close(self, old_kf, res, pixels):
        n = len(self.keyframes) - 1
        self.X.append(self.X[n - 1] @ res["T"].astype(np.float64))
        self.edges.append((n - 1, n, res["T"].astype(np.float64), information(res["sums"])))
        self.db[n - 1] = old_kf
        if len(self.db) > self.lp["keep"]:
            del self.db[min(self.db)]
        cands = select_candidates(self.X, n, list(self.db), self.lp["gap"], self.lp["radius"], self.lp["angle"], self.lp["cap"])
        accepted, applied = [], False
        for k, G in cands:
            r = R.align(self.db[k], self.kf, G.astype(np.float32), self.lp["iters"], self.lp["dist_th"], self.normal_th_deg,
                        int(np.ceil(self.min_pairs_frac * pixels)), self.min_pivot_ratio, self.dtype)
            self._n_align += 1
            if accept(r, G.astype(np.float32), pixels, self.lp["overlap"], self.lp["rms"], self.lp["corr"]):
                self.edges.append((k, n, r["T"].astype(np.float64), information(r["sums"])))
                self.edges_accepted.append((k, n))
                accepted.append(k)
        if accepted:
            c0 = cost(self.X, self.edges)
            if self.solver is None:
                X, c = minimise(self.X, self.edges)
                improved = c < c0
            else:
                X, improved = self.solver(self.X, self.edges)
            moved = [R.pose_distance(a, b) for a, b in zip(self.X, X)]
            if improved and any(t > self.lp["shift"][0] or a > self.lp["shift"][1] for t, a in moved):
                self.X = X
                for i, x in enumerate(X):
                    self.keyframes[i] = np.concatenate([self.keyframes[i][:1], x.astype(np.float32)[:3].reshape(12)])
                self.kf_c2w = self.c2w = X[n].astype(np.float32)
                self.rows[-1] = self.keyframes[n]
                self.big += 1
                applied = True
        self.attempts.append((n, [k for k, _ in cands], accepted, applied))
