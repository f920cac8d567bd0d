"""CPU restatement of kin_traj_opt_scene_batch (include/kinhip.h; the kernel is k_traj_scene, kinhip_traj_dev.h with
SCENE != 0): tests/trajopt_ref.py's merit() and run(), unchanged, on a scene whose boxes ride on a scene mechanism
and whose every waypoint has its own scene state.  Not a test module: imported by tests/trajopt_scene_cases.py,
tests/test_trajopt_scene.py and tests/test_gpu_traj_scene.py.

AttachedScene overrides SceneBase.distances(Q): the world pose of box k at sample n is
get_transform(scene, link_k) * origin_k from an OracleMech of the scene at that sample's scene values (its batched
driver fk_batch, one configuration per sample), and every sample's poses go to trajopt_ref.union_box_sdf in the
kernel's order: group after group (a group = the boxes behind the same last scene batch joint, the root group for
none; groups in the order of their first box), the boxes of a group in link order.

merit() and run() hand distances() the columns of the live trajectories only, without saying which they are; the
end waypoints of a trajectory never change during a solve, so bind() records (start, goal) -> trajectory and
distances() finds each block of n_wp columns by its end columns.  With one scene state for the whole launch
(scene_q of shape (n_scene_cols,)) nothing is looked up."""
import numpy as np

import oracle as O
import trajopt_ref as R


def pose_of(p12):
    """[12, N] (3x4 column-major) -> [N, 4, 4]."""
    N = p12.shape[1]
    T = np.zeros((N, 4, 4))
    T[:, :3, :3] = np.transpose(p12[:9].reshape(3, 3, N), (2, 1, 0))     # R[i][j] = p[i + 3 j]
    T[:, :3, 3] = p12[9:12].T
    T[:, 3, 3] = 1.0
    return T


def box_groups(tree, scene_ids):
    """The kernel's box order for UnionSDF(scene): [(link id, origin 4x4, widths)] group after group, and each box's
    group (0-based, by first appearance) and whether that group moves (kin_sdf_create_attached)."""
    batch = {int(j) for j in scene_ids if tree.joint_type[int(j) - 1] != O.FIXED}
    pj = {int(c): k + 1 for k, c in enumerate(tree.joint_clink)}
    keys, boxes = [], []
    for lid, (ext, org) in sorted(tree.link_box.items()):
        key, x = -1, int(lid)
        while x in pj:                 # the last batch joint on the root path = the first met walking up
            if pj[x] in batch:
                key = pj[x]
                break
            x = int(tree.joint_plink[pj[x] - 1])
        if key not in keys:
            keys.append(key)
        boxes.append((keys.index(key), int(lid), np.asarray(org, np.float64), tuple(float(e) for e in ext)))
    order = sorted(range(len(boxes)), key=lambda k: (boxes[k][0], k))
    out = [boxes[k][1:] for k in order]
    grp = [boxes[k][0] for k in order]
    return out, grp, [k != -1 for k in keys]


class AttachedScene(R.SceneBase):
    """robot: a SceneBase (om, ids, sph, rad, lo, hi, n_dof); scene_tree / scene_base / scene_ids: the scene
    mechanism, whether it has the planar base, its batch joints in column order (scene_q rows: the joints, then base
    x, y, theta).  Other scene joints stay at 0."""

    def __init__(self, robot, scene_tree, scene_base, scene_ids):
        for k in ("om", "ids", "sph", "rad", "lo", "hi", "n_dof", "with_base", "tree"):
            setattr(self, k, getattr(robot, k))
        self.robot = robot
        self.scene_tree, self.scene_base = scene_tree, bool(scene_base)
        self.scene_ids = [int(j) for j in scene_ids]
        self.som = O.OracleMech(scene_tree, with_base=scene_base)
        self.boxes, self.box_group, self.group_moves = box_groups(scene_tree, self.scene_ids)
        self.box_widths = [b[2] for b in self.boxes]
        self.n_scene_cols = len(self.scene_ids) + (3 if scene_base else 0)
        self.n_wp, self.SQ, self._by_ends = None, None, {}

    # ---- the scene state of every sample -------------------------------------------------------------------
    def bind(self, X0, SQ):
        """X0 [nt, n_wp, nd]; SQ (n_scene_cols,) for the whole launch or (n_scene_cols, nt * n_wp), column
        t * n_wp + w.  Returns self."""
        nt, n_wp, _ = X0.shape
        SQ = np.asarray(SQ, np.float64)
        assert SQ.shape in ((self.n_scene_cols,), (self.n_scene_cols, nt * n_wp)), SQ.shape
        self.n_wp, self.SQ, self._by_ends = n_wp, SQ, {}
        for t in range(nt):
            self._by_ends.setdefault(X0[t, 0].tobytes() + X0[t, -1].tobytes(), t)
        return self

    def samples_of(self, Q):
        """The scene columns [n_scene_cols, N] of the columns of Q (whole trajectories, found by their ends)."""
        N = Q.shape[1]
        if self.SQ.ndim == 1:
            return np.repeat(self.SQ[:, None], N, axis=1)
        assert N % self.n_wp == 0, "distances(): whole trajectories only (distances_at takes any columns)"
        out = np.zeros((self.n_scene_cols, N))
        for b in range(N // self.n_wp):
            c0 = b * self.n_wp
            t = self._by_ends[np.ascontiguousarray(Q[:, c0]).tobytes()
                              + np.ascontiguousarray(Q[:, c0 + self.n_wp - 1]).tobytes()]
            out[:, c0:c0 + self.n_wp] = self.SQ[:, t * self.n_wp:(t + 1) * self.n_wp]
        return out

    # ---- geometry ------------------------------------------------------------------------------------------
    def world_boxes(self, SQ):
        """SQ [n_scene_cols, N] -> [N, n_box, 4, 4]: get_transform(scene, link) * origin per sample, kernel order."""
        SQ = np.ascontiguousarray(np.asarray(SQ, np.float64).reshape(self.n_scene_cols, -1))
        links = [b[0] for b in self.boxes]
        poses = self.som.fk_batch(SQ, self.scene_ids, links)               # [n_box, 12, N]
        return np.stack([pose_of(poses[k]) @ self.boxes[k][1] for k in range(len(links))], axis=1)

    def centres(self, Q):
        poses = self.om.fk_batch(Q, self.ids, self.sph)                    # [n_sph, 12, N]
        return np.transpose(poses[:, 9:12, :], (0, 2, 1))                  # [n_sph, N, 3]

    def distances_at(self, Q, SQ):
        """Q [n_dof, N], SQ [n_scene_cols, N] -> sphere distances [n_sph, N], SDF gradients [n_sph, N, 3]."""
        C = self.centres(Q)
        WB = self.world_boxes(SQ)
        ns, N = C.shape[0], C.shape[1]
        d, g = np.zeros((ns, N)), np.zeros((ns, N, 3))
        for n in range(N):
            d[:, n], g[:, n] = R.union_box_sdf(C[:, n], list(WB[n]), self.box_widths)
        return d - self.rad[:, None], g

    def distances(self, Q):
        return self.distances_at(Q, self.samples_of(Q))

    def per_box(self, Q, SQ):
        """Every box's own distance [n_box, n_sph, N] (minus the radius): the conditions on the cases."""
        C = self.centres(Q)
        WB = self.world_boxes(SQ)
        out = np.zeros((len(self.boxes), C.shape[0], C.shape[1]))
        for n in range(C.shape[1]):
            for k in range(len(self.boxes)):
                out[k, :, n] = R.union_box_sdf(C[:, n], [WB[n, k]], [self.box_widths[k]])[0]
        return out - self.rad[None, :, None]

    def frozen(self, state):
        """The static snapshot at one scene state (n_scene_cols,): a SceneBase with world box poses (kernel order)."""
        sc = R.SceneBase()
        for k in ("om", "ids", "sph", "rad", "lo", "hi", "n_dof", "with_base", "tree"):
            setattr(sc, k, getattr(self, k))
        sc.box_poses = list(self.world_boxes(np.asarray(state, np.float64).reshape(-1, 1))[0])
        sc.box_widths = list(self.box_widths)
        return sc
