"""Scan of a gripper at a joint state (reference: mgs/env/gripper_scan.py:52-103
with MjScanEnv.scan, mgs/env/base.py:77-126, and mgs/cli/scan_gripper.py).

The gripper's own MJCF is compiled alone -- no table, no objects -- and drawn
from Fibonacci views over the whole sphere by the ray caster behind
ClutterTableEnv.scan (mgs_scan_render).  This build ships no visual meshes, so
what is drawn is the collision geometry the engine simulates: one drawable per
compiled geom (box, sphere, capsule, cylinder; a mesh geom as its convex hull),
posed by the host kinematics of mgs/scan/kin.py.  A segmentation id is the
geom's index in the compiled model.

Segments follow the rule the reference's hand-kept `segmentation:` id lists
encode -- every list is "the geoms joint j moves": one segment per hinge or
slide joint holding the geoms of the joint's body and of everything below it,
and `body` for the whole gripper.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from mgs.core.mjcf import GEOM_TYPES, CompiledModel, compile_xml
from mgs.scan import camera, kin
from mgs.util.geo.transforms import SE3Pose

# the options of the reference's template (gripper_scan.py:26-36); its centre
# marker (a 1 um sphere), camera body and lights are render-only and not compiled
XML = r"""
<mujoco>
    <compiler angle="radian" autolimits="true" />
    <option integrator="implicitfast" timestep="0.001"/>
    <option><flag multiccd="enable"/> </option>
    <option cone="elliptic" gravity="0 0 0" impratio="3" timestep="0.001" noslip_iterations="2" noslip_tolerance="1e-8" tolerance="1e-8"/>
    {gripper}
</mujoco>
"""

SCAN_TARGET = np.zeros(3)                 # the reference's `center` body
CLOUD_REGION = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
CLOUD_BUCKET = 0.016                      # the pick's bucket side, as the scene cloud's (8 x 2 mm)
_TYPE_NAME = {v: k for k, v in GEOM_TYPES.items()}


class GripperScanEnv:
    def __init__(self, gripper, device: int = 0):
        self.gripper = gripper
        self.device = device
        self.gripper_xml, self.gripper_assets = gripper.to_xml()
        self.model_xml = XML.format(gripper=self.gripper_xml)
        self.model: CompiledModel = compile_xml(self.model_xml, dict(self.gripper_assets))
        cm = self.model
        self.qpos = cm.qpos0.copy()
        # gripper_scan.py:86-91: set_pose(identity @ base_to_contact)
        pose = SE3Pose(np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0]), type="wxyz")
        self.set_pose(pose @ gripper.base_to_contact_transform())
        self.scan_width = self.scan_height = 480
        self._scan_cam = None
        self._hull_faces = {}
        self.last_scan = None

    # -- state ------------------------------------------------------------------
    def get_joint_idxs(self, joint_list: List[str]) -> List[int]:
        return [self.model.jnt_qposadr_by_name(j) for j in joint_list]

    def set_qpos(self, values, idxs) -> None:
        for v, a in zip(np.asarray(values, np.float64).reshape(-1), idxs):   # sequential: duplicates -> last wins
            self.qpos[int(a)] = v

    def set_pose(self, pose: SE3Pose) -> None:
        """the free joint's qpos from a processed pose (gripper/base.py:48-59)"""
        vec = np.asarray(pose.to_vec(layout="pq", type="wxyz"), np.float64).reshape(-1)
        a = self.model.jnt_qposadr_by_name("freejoint")
        self.qpos[a:a + 7] = vec[:7]

    def _sizes(self):
        """the integration-state layout of ClutterTableEnv for the reference's
        scan model: the gripper's joints, then the camera's free joint; two
        more bodies (centre marker, camera)"""
        cm = self.model
        nq, nv, nb = cm.nq + 7, cm.nv + 6, cm.nbody + 2
        return [("time", 1), ("qpos", nq), ("qvel", nv), ("act", int(cm.nact)), ("qacc_warmstart", nv),
                ("ctrl", cm.nu), ("qfrc_applied", nv), ("xfrc_applied", 6 * nb), ("eq_active", len(cm.eq_type)),
                ("mocap_pos", 3), ("mocap_quat", 4)]

    def state_size(self) -> int:
        return sum(n for _, n in self._sizes())

    def set_state(self, state) -> None:
        """only the gripper's qpos of the state matters for a scan"""
        state = np.asarray(state, np.float64)
        if state.shape != (self.state_size(),):
            raise ValueError(f"state has {state.shape[0] if state.ndim else 0} entries, expected {self.state_size()} "
                             "(mjSTATE_INTEGRATION of the scan model)")
        self.qpos = state[1:1 + self.model.nq].copy()

    def get_state(self) -> np.ndarray:
        cm = self.model
        parts = {k: np.zeros(n) for k, n in self._sizes()}
        parts["qpos"] = np.concatenate([self.qpos, [0.0, 0.0, 0.4, 1.0, 0.0, 0.0, 0.0]])   # camera body, :42
        parts["eq_active"][:] = 1.0
        m = cm.body_names.index("mocap") if "mocap" in cm.body_names else None
        if m is not None:
            parts["mocap_pos"], parts["mocap_quat"] = cm.body_pos[m], cm.body_quat[m]
        return np.concatenate([np.asarray(parts[k], np.float64).reshape(n) for k, n in self._sizes()])

    # -- scene --------------------------------------------------------------------
    @property
    def scan_geom_names(self) -> List[str]:
        """what a segmentation id indexes: the compiled model's geoms, in model order"""
        return list(self.model.geom_names)

    def scan_scene(self):
        """one drawable per compiled geom at the pose of the joint state"""
        from mgs.core.mjcf import _hull_faces
        from mgs.scan.scene import ScanScene
        cm = self.model
        pos, rot = kin.geom_poses(cm, self.qpos)
        sc = ScanScene()
        for g in range(len(cm.geom_bodyid)):
            t, size = _TYPE_NAME[int(cm.geom_type[g])], cm.geom_size[g]
            if t == "box":
                sc.add_box(g, pos[g], rot[g], size)
            elif t == "sphere":
                sc.add_sphere(g, pos[g], size[0])
            elif t == "capsule":
                sc.add_capsule(g, pos[g], rot[g], size[0], size[1])
            elif t == "cylinder":
                sc.add_cylinder(g, pos[g], rot[g], size[0], size[1])
            elif t == "mesh":
                h = int(cm.geom_hullid[g])
                a, n = int(cm.hull_vertadr[h]), int(cm.hull_vertnum[h])
                verts = cm.hull_vert[a:a + n]
                if h not in self._hull_faces:
                    self._hull_faces[h] = _hull_faces(verts)
                sc.add_mesh(g, pos[g], rot[g], verts, self._hull_faces[h], key=h)
            else:
                raise NotImplementedError(f"geom {g} ({cm.geom_names[g]!r}): a {t} is not drawn")
        return sc

    # -- camera -------------------------------------------------------------------
    def update_camera_settings(self, num_images, i):
        """view i of num_images: the unit Fibonacci point (not lifted: the views
        cover the whole sphere, gripper_scan.py:93-97), looking at the origin
        by MuJoCo's `targetbody` rule (restated: mgs.scan.scene.look_at_frame)"""
        from mgs.scan.scene import look_at_frame
        from mgs.util.camera import fibonacci_sphere
        pos = fibonacci_sphere(total_num=num_images, i=i)
        self._scan_cam = (pos, look_at_frame(pos, SCAN_TARGET))

    def get_camera_extrinsics(self) -> np.ndarray:
        if self._scan_cam is None:
            from mgs.scan.scene import look_at_frame
            p = np.array([0.0, 0.0, 0.4])                                    # the camera body's load pose, :42
            self._scan_cam = (p, look_at_frame(p, SCAN_TARGET))
        return camera.extrinsics(*self._scan_cam)

    def get_camera_intrinsics(self) -> np.ndarray:
        return camera.reference_intrinsics(self.scan_width, self.scan_height)

    def get_render_intrinsics(self) -> np.ndarray:
        return camera.render_intrinsics(self.scan_width, self.scan_height)

    # -- scan ---------------------------------------------------------------------
    def scan(self, num_images=1, width=480, height=480):
        """as ClutterTableEnv.scan: (rgbd (N, H, W, 4) float32 -- flat 0.5 grey
        and planar depth, 0 where nothing is hit --, extrinsics (N, 4, 4),
        image_masks (N, H, W) bool: the hit mask eroded 5 times, segmentation
        (N, H, W) int32: index into scan_geom_names, -1 = nothing).  `last_scan`
        keeps the f64 depth, seg, face ids, extrinsics and the kernel time."""
        from mgs.core.engine import scan_render
        from mgs.scan.scene import erode_mask
        self.scan_width, self.scan_height = int(width), int(height)
        extr = []
        for i in range(num_images):
            self.update_camera_settings(num_images, i)
            extr.append(self.get_camera_extrinsics())
        extr = np.stack(extr, axis=0) if extr else np.zeros((0, 4, 4))
        K = self.get_render_intrinsics()
        res = scan_render(self.scan_scene().arrays(), extr[:, :3, 3], extr[:, :3, :3], width, height,
                          K[0, 0], K[1, 1], K[0, 2], K[1, 2], device=self.device)
        seg = res["seg"]
        colors = np.concatenate([np.full((len(self.scan_geom_names), 3), 0.5), np.zeros((1, 3))]).astype(np.float32)
        rgbd = np.concatenate([colors[seg], res["depth"].astype(np.float32)[..., None]], axis=-1)
        masks = erode_mask(seg != -1, 5)
        self.last_scan = dict(res, extrinsics=extr, image_masks=masks)
        return rgbd, extr, masks, seg

    def _segment_geoms(self, spec=None):
        """(names, geom index arrays) of the segments"""
        cm = self.model
        if spec is None:
            joints = [n for n, t in zip(cm.jnt_names, cm.jnt_type) if int(t) in (kin.SLIDE, kin.HINGE)]
            names, geoms = list(joints), [kin.moved_geoms(cm, j) for j in joints]
            names.append("body")
            geoms.append(np.arange(len(cm.geom_bodyid)))
            return names, geoms
        names, geoms = [], []
        for name, joint in dict(spec).items():
            names.append(str(name))
            geoms.append(kin.moved_geoms(cm, joint))      # ValueError on an unknown joint
        return names, geoms

    def segments(self, segmentation, image_masks, spec=None):
        """(names, masks (nseg, N, H, W) bool): per segment the pixels of the
        geoms its joint moves, inside image_masks.  Default: one segment per
        hinge or slide joint, named by the joint, then `body` (every geom);
        `spec` maps segment name -> joint name (config key gripper.segmentation)."""
        names, geoms = self._segment_geoms(spec)
        seg, keep = np.asarray(segmentation), np.asarray(image_masks, bool)
        masks = np.zeros((len(names),) + seg.shape, bool)
        for k, g in enumerate(geoms):
            masks[k] = np.isin(seg, g) & keep
        return names, masks

    def cloud(self, num_points, region=None, spec=None):
        """the last scan as points (what the reference's kinematic_pcd_transform
        poses by per-joint masks): mgs_scan_points with the reference's
        intrinsics, erosion 5 and `region` (lo xyz, hi xyz; default +-0.5 m),
        the kept points in (view, row, column) order and, with more than
        num_points of them, the farthest-point pick (mgs_scan_fps) of the
        float32-rounded points.  Returns points float32 (P, 3), point_geom int32
        (P,) -- each point's pixel's segmentation id -- and point_segments bool
        (nseg, P) in the order of segments()."""
        from mgs.core.engine import scan_fps, scan_points
        if self.last_scan is None:
            raise RuntimeError("cloud() uses the last scan: call scan() first")
        res = self.last_scan
        K = self.get_camera_intrinsics()
        region = CLOUD_REGION if region is None else np.asarray(region, np.float64).reshape(6)
        pts, keep, _ = scan_points(res["depth"], res["seg"], res["extrinsics"], K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                   erode_iters=5, region=region, device=self.device)
        points, geom = pts[keep].astype(np.float32), res["seg"][keep].astype(np.int32)
        if len(points) > int(num_points):
            idx, _, _ = scan_fps(points.astype(np.float64), int(num_points), CLOUD_BUCKET, device=self.device)
            points, geom = points[idx], geom[idx]
        _, geoms = self._segment_geoms(spec)
        member = np.stack([np.isin(geom, g) for g in geoms]) if geoms else np.zeros((0, len(geom)), bool)
        return points, geom, member

    # -- posing ---------------------------------------------------------------------
    def kinematic_tree(self):
        """the model's hinge and slide joints as a mgs.sampler.kin.tree
        KinematicTree at the current free-joint pose; theta_scan is the current
        joint state (what a scan taken now shows)"""
        from mgs.sampler.kin.tree import tree_from_model
        return tree_from_model(self.model, self.qpos)

    def pose_cloud(self, points, point_geom, joints, poses=None, dtype=np.float32, points_per_group=0):
        """the cloud of cloud() -- scanned at the current joint state -- at B
        joint states on the GPU (mgs_pose_cloud).  joints (B, nlink): theta =
        qpos - qpos0 per link of kinematic_tree() (tree.theta_from_qpos /
        theta_from_named build it); poses (B, 4, 4): grasp poses in the contact
        frame, which is the scan's world frame (set_pose at identity @
        base_to_contact_transform()), so the scene-frame cloud is pose_b . p.
        Returns dict(points (B, P, 3) of dtype, links, kernel_ms, point_link)."""
        from mgs.core.engine import pose_cloud
        tree = self.kinematic_tree()
        geom = np.asarray(point_geom, np.int64).reshape(-1)
        if len(geom) and (geom.min() < 0 or geom.max() >= len(self.model.geom_bodyid)):
            raise ValueError("point_geom holds an index that is no geom of the model")
        link = tree.link_of_geoms(self.model)[geom]
        res = pose_cloud(tree, points, link, joints, base=poses, dtype=dtype, points_per_group=points_per_group,
                         device=self.device)
        return dict(res, point_link=link)
