"""Re-fusion after a loop closure restated in plain numpy from the contract's text, on top of tests/tsdf_restatement.py and
tests/loop_restatement.py (neither is changed):

  history_poses      TsdfHistory.poses: X[kf] @ rel in f64, rounded to f32 once
  ModelLoopTracker   tsdf_restatement.ModelTracker with a history, the six steps of close_loops on every new keyframe (the keyframes' OWN depth images
                     verified against each other, the odometry edge keyframe to keyframe) and, on an applied closure, the volume fused again from the
                     history and the model image cast at the corrected pose.  f64 and f32 forms; the graph is f64 in both."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402
import loop_restatement as LR  # noqa: E402
import tsdf_restatement as T  # noqa: E402


def history_poses(entries, X):
    return [(np.asarray(X[e["kf"]], np.float64) @ np.asarray(e["rel"], np.float64)).astype(np.float32) for e in entries]


class ModelLoopTracker(T.ModelTracker):
    """Records, beside ModelTracker's: `big_change` per frame, `attempts` (n, candidates, accepted, applied) per new keyframe, `edges_accepted`,
    `keyframes` (rows, as corrected), `kf_history` (the keyframe rows after each frame), `loop_results` (per attempt: [(k, G, result)]), `history`
    (entries {"frame", "depth", "kf", "rel"}, oldest first) and `steps`: how many alignments stand behind each frame's pose."""

    def __init__(self, K, sp, near, far, history, loop_min_gap=10, loop_radius=0.5, loop_angle_deg=30.0, loop_max_candidates=8, loop_iters=None,
                 loop_dist_th=0.2, loop_min_overlap=0.3, loop_max_rms=0.02, loop_max_correction=(0.3, 10.0), loop_min_shift=(0.01, 0.2), **kw):
        super().__init__(K, sp, near, far, **kw)
        self.lp = dict(gap=loop_min_gap, radius=loop_radius, angle=loop_angle_deg, cap=loop_max_candidates, iters=loop_iters or self.iters,
                       dist_th=loop_dist_th, overlap=loop_min_overlap, rms=loop_max_rms, corr=loop_max_correction, shift=loop_min_shift)
        self.capacity, self.history = int(history), []
        self.X, self.edges, self.db, self.kf = [np.eye(4)], [], {}, None
        self.big, self.big_change, self.attempts, self.edges_accepted, self.keyframes, self.kf_history = 0, [], [], [], [], []
        self.loop_results, self.steps, self._n_align = [], [], 0

    def _keep(self, t, depth, kf, rel):
        self.history = (self.history + [{"frame": t, "depth": depth, "kf": kf, "rel": np.array(rel, dtype=np.float64)}])[-self.capacity:]

    def process(self, depth, t):
        self._process(depth, t)
        self.big_change.append(self.big)
        self.steps.append(self._n_align)
        self.kf_history.append(list(self.keyframes))

    def _process(self, depth, t):
        if self.vol is None:
            self.vol = T.empty(self.sp, self.dtype)
            self.kf = R.prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)      # the first keyframe's own image
            self.rows.append(self._row(t)); self.flags.append(True); self.states.append(R.OK); self.margins.append(None); self.results.append(None)
            self.keyframes.append(self.rows[-1])
            self._keep(t, depth, 0, np.eye(4))
            self._fuse(depth)
            return
        cur = R.prepare(depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
        pixels = depth.shape[0] * depth.shape[1]
        min_pairs = int(np.ceil(self.min_pairs_frac * pixels))
        res = R.align(self.model, cur, np.eye(4, dtype=np.float32), self.iters, self.dist_th, self.normal_th_deg, min_pairs, self.min_pivot_ratio, self.dtype)
        self.results.append(res)
        if res["state"] != R.OK:                             # pose, volume, model image and history stay
            self.rows.append(self.rows[-1]); self.flags.append(False); self.states.append(R.LOST); self.margins.append(None)
            return
        self._n_align += 1
        self.c2w = (self.c2w.astype(np.float64) @ res["T"].astype(np.float64)).astype(np.float32)
        rel = np.linalg.inv(self.kf_c2w.astype(np.float64)) @ self.c2w.astype(np.float64)
        tr, rot = R.pose_distance(np.eye(4), rel)
        self.margins.append({"translation": tr, "rotation": rot, "pairs": res["pairs"], "pixels": pixels})
        kf = bool(R.keyframe_decision(rel, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap))
        self.rows.append(self._row(t)); self.flags.append(kf); self.states.append(R.OK)
        if kf:
            self.kf_c2w = self.c2w
            self.keyframes.append(self.rows[-1])
        self._keep(t, depth, len(self.keyframes) - 1, np.eye(4) if kf else rel)
        self._fuse(depth)                                    # at the uncorrected pose, as every OK frame
        if kf:
            old, self.kf = self.kf, cur
            self._close(old, res, rel, pixels, min_pairs)

    def _close(self, old_kf, res, rel, pixels, min_pairs):
        n = len(self.keyframes) - 1
        self.X.append(self.X[n - 1] @ rel)                   # keyframe to keyframe; the information is that of the alignment to the model
        self.edges.append((n - 1, n, rel, LR.information(res["sums"])))
        self.db[n - 1] = old_kf
        cands = LR.select_candidates(self.X, n, list(self.db), self.lp["gap"], self.lp["radius"], self.lp["angle"], self.lp["cap"])
        accepted, applied, results = [], False, []
        for k, G in cands:
            r = R.align(self.db[k], self.kf, G.astype(np.float32), self.lp["iters"], self.lp["dist_th"], self.normal_th_deg, min_pairs,
                        self.min_pivot_ratio, self.dtype)
            self._n_align += 1
            results.append((k, G, r))
            if LR.accept(r, G.astype(np.float32), pixels, self.lp["overlap"], self.lp["rms"], self.lp["corr"]):
                self.edges.append((k, n, r["T"].astype(np.float64), LR.information(r["sums"])))
                self.edges_accepted.append((k, n))
                accepted.append(k)
        if accepted:
            c0 = LR.cost(self.X, self.edges)
            X, c = LR.minimise(self.X, self.edges)
            moved = [R.pose_distance(a, b) for a, b in zip(self.X, X)]
            if c < c0 and any(t > self.lp["shift"][0] or a > self.lp["shift"][1] for t, a in moved):
                self.X = X
                for i, x in enumerate(X):
                    self.keyframes[i] = np.concatenate([self.keyframes[i][:1], x.astype(np.float32)[:3].reshape(12)])
                self.kf_c2w = self.c2w = X[n].astype(np.float32)
                self.rows[-1] = self.keyframes[n]
                self.big += 1
                applied = True
                self._refuse()
        self.attempts.append((n, [k for k, _ in cands], accepted, applied))
        self.loop_results.append(results)

    def _refuse(self):
        """The volume again from the history at the corrected poses, in order; the model image at the corrected pose."""
        self.vol = T.empty(self.sp, self.dtype)
        h, w = self.history[0]["depth"].shape
        for e, pose in zip(self.history, history_poses(self.history, self.X)):
            cam = T.camera(self.K, h, w, pose, self.near, self.far)
            box = T.frustum_box(self.sp, cam)
            if box is not None:
                T.integrate(self.vol, self.sp, e["depth"], cam, box, self.dtype)
        cam = T.camera(self.K, h, w, self.c2w, self.near, self.far)
        self.model_depth = T.raycast(self.vol, self.sp, cam, self.sp["trunc"] / np.float32(2), self.dtype, knife_edges=False)[0].astype(np.float32)
        self.model = R.prepare(self.model_depth, self.K, self.levels, self.max_depth, self.depth_jump, self.dtype)
