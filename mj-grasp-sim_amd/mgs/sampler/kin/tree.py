"""Kinematic trees for posing a scanned gripper cloud by joint values
(csrc/mgs_pose.hip through mgs.core.engine.pose_cloud).

A tree is data.  Link i hangs from link parent[i] < i or from the base (-1);
kin_tf[i] takes the parent's link frame to link i's rest frame (unit quaternion
wxyz + xyz), joint_tf[i] holds the prismatic direction and the revolute axis in
that frame, and

    W_i(theta) = W_parent(i)(theta) o kin_tf[i] o J_i(theta_i),   W_base = identity,

with J_i = (quaternion_from_axis_angle(axis, theta_i), direction * theta_i) and
the identity quaternion for an axis of norm 0, as the reference's
kinematic_pcd_transform forms them (mgs/sampler/kin/base.py:56-72).  A cloud
scanned at theta_scan is posed at theta by moving every point with the
transform of the link it is fixed to, W_i(theta) o W_i(theta_scan)^-1.

Two sources: the hand-kept table of the contact sampler (tree_from_kinematics,
the Shadow Hand of mgs.sampler.kin.model) and any compiled gripper model
(tree_from_model: the hinge and slide joints of the MJCF body tree).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from mgs.core.mjcf import quat2mat, quat_conj, quat_mul
from mgs.scan import kin as scan_kin

MAXLINK = 32
FREE_JOINT = "freejoint"      # the gripper's own free joint (mgs.gripper.base)


@dataclass
class KinematicTree:
    parent: np.ndarray               # (nlink,) int32, -1 = the base
    kin_tf: np.ndarray               # (nlink, 7) parent link frame -> rest frame, unit wxyz + xyz
    joint_tf: np.ndarray             # (nlink, 6) prismatic direction, revolute axis, link frame
    joint_names: List[str]
    theta_scan: np.ndarray           # (nlink,) the joint values the cloud was scanned at
    # trees of a compiled model: where each link's joint sits in qpos, its qpos0,
    # and the link (1 + index, 0 = base) every body is fixed to
    qposadr: Optional[np.ndarray] = None
    qpos0: Optional[np.ndarray] = None
    body_link: Optional[np.ndarray] = field(default=None, repr=False)

    def __post_init__(self):
        self.parent = np.ascontiguousarray(self.parent, np.int32).reshape(-1)
        n = len(self.parent)
        self.kin_tf = np.ascontiguousarray(self.kin_tf, np.float64).reshape(n, 7)
        self.joint_tf = np.ascontiguousarray(self.joint_tf, np.float64).reshape(n, 6)
        self.theta_scan = np.ascontiguousarray(self.theta_scan, np.float64).reshape(n)
        self.joint_names = [str(s) for s in self.joint_names]
        if not 1 <= n <= MAXLINK:
            raise ValueError(f"a kinematic tree has 1 .. {MAXLINK} links, not {n}")
        if len(self.joint_names) != n:
            raise ValueError(f"{len(self.joint_names)} joint names for {n} links")
        for i, p in enumerate(self.parent):
            if not -1 <= p < i:
                raise ValueError(f"parent[{i}] = {p}: a link hangs from an earlier link or from the base (-1)")

    @property
    def nlink(self) -> int:
        return len(self.parent)

    def _rest(self):
        return np.zeros(self.nlink) if self.qpos0 is None else self.qpos0

    def theta_from_qpos(self, qpos) -> np.ndarray:
        """theta (..., nlink) = qpos - qpos0 at the links' joints (trees of a model)"""
        if self.qposadr is None:
            raise ValueError("theta_from_qpos: this tree was not built from a compiled model")
        return np.asarray(qpos, np.float64)[..., self.qposadr] - self.qpos0

    def theta_from_named(self, values, names) -> np.ndarray:
        """theta (..., nlink) from joint positions `values` (..., len(names)) of
        the joints `names`: value - qpos0 there, 0 (the rest position) at every
        other joint"""
        values = np.asarray(values, np.float64)
        names = [str(s) for s in names]
        if values.shape[-1:] != (len(names),):
            raise ValueError(f"{values.shape[-1] if values.ndim else 0} values for {len(names)} joint names")
        theta = np.zeros(values.shape[:-1] + (self.nlink,))
        rest = self._rest()
        for k, name in enumerate(names):
            if name not in self.joint_names:
                raise ValueError(f"unknown joint {name!r} (the tree has {self.joint_names})")
            i = self.joint_names.index(name)
            theta[..., i] = values[..., k] - rest[i]
        return theta

    def link_of_geoms(self, cm) -> np.ndarray:
        """(ngeom,) int32 in [0, nlink]: 0 = the base, k = link k - 1 -- the last
        hinge or slide joint on the geom's body, else that of the nearest
        ancestor body that has one"""
        if self.body_link is None:
            raise ValueError("link_of_geoms: this tree was not built from a compiled model")
        return self.body_link[np.asarray(cm.geom_bodyid, np.int64)].astype(np.int32)

    def links_from_segments(self, masks, order=None) -> np.ndarray:
        """(P,) int32 in [0, nlink] from the reference's representation, one bool
        mask per joint (`order`: the joint name of each row; default: the
        tree's).  A point's link is the deepest joint whose mask holds it; its
        set of masks must be exactly that link and its ancestors -- only then
        do the reference's sequential masked transforms equal one transform by
        that link -- else ValueError."""
        masks = np.asarray(masks, bool)
        order = self.joint_names if order is None else [str(s) for s in order]
        if masks.ndim != 2 or masks.shape[0] != len(order):
            raise ValueError(f"masks {masks.shape}: one row per joint of {len(order)} expected")
        member = np.zeros((self.nlink, masks.shape[1]), bool)
        for row, name in zip(masks, order):
            if name not in self.joint_names:
                raise ValueError(f"unknown joint {name!r} (the tree has {self.joint_names})")
            member[self.joint_names.index(name)] |= row
        link = np.zeros(masks.shape[1], np.int32)
        for i in range(self.nlink):      # parents come first: the last hit is the deepest
            link[member[i]] = i + 1
        want = np.zeros_like(member)
        for i in range(self.nlink):
            on, a = link == i + 1, i
            while a >= 0:
                want[a] |= on
                a = int(self.parent[a])
        bad = np.nonzero((want != member).any(axis=0))[0]
        if len(bad):
            p = int(bad[0])
            have = [self.joint_names[i] for i in np.nonzero(member[:, p])[0]]
            need = [self.joint_names[i] for i in np.nonzero(want[:, p])[0]]
            raise ValueError(f"{len(bad)} point(s) whose masks are not a link and its ancestors; point {p} is in "
                             f"{have}, its deepest link needs {need}")
        return link


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


def tree_from_kinematics(kin, theta_scan=None) -> KinematicTree:
    """the tree of a KinematicsModel table (mgs.sampler.kin.model).  The table's
    quaternions are normalised here: they are off unit length by 2.7e-7 and the
    posing takes the conjugate for the inverse, as the reference's se3_invert."""
    n = kin.num_dofs
    kt = np.array(kin.kin_tf, np.float64)
    kt[:, :4] = _unit(kt[:, :4])
    return KinematicTree(parent=kin.parents(), kin_tf=kt, joint_tf=np.array(kin.joint_tf, np.float64),
                         joint_names=[f"dof{i}" for i in range(n)],
                         theta_scan=np.zeros(n) if theta_scan is None else theta_scan)


def tree_from_model(cm, qpos=None) -> KinematicTree:
    """the tree of a compiled gripper model: one link per hinge or slide joint
    that is not under a foreign free joint (any but the gripper's own
    `freejoint`), in model joint order.  Link i's rest frame is the orientation
    of the joint's body with its origin at the joint anchor, at qpos0 of the
    non-free joints and the free-joint pose of `qpos` (default qpos0); its
    parent is the previous hinge or slide joint on the same body, else the last
    one of the nearest ancestor body that has one, else the base.  theta is
    qpos - qpos0; theta_scan comes from `qpos`.  Closed loops are not solved:
    this is the spanning tree and the caller supplies every joint."""
    qpos = cm.qpos0.copy() if qpos is None else np.asarray(qpos, np.float64).reshape(-1)
    if qpos.shape != (cm.nq,):
        raise ValueError(f"qpos has {qpos.shape[0]} entries, the model has nq = {cm.nq}")
    rest = cm.qpos0.copy()
    foreign = np.zeros(cm.nbody, bool)
    for b in range(1, cm.nbody):
        foreign[b] = foreign[int(cm.body_parentid[b])]
        for j in range(int(cm.body_jntadr[b]), int(cm.body_jntadr[b]) + int(cm.body_jntnum[b])):
            t, a = int(cm.jnt_type[j]), int(cm.jnt_qposadr[j])
            if t == scan_kin.FREE:
                rest[a:a + 7] = qpos[a:a + 7]
                if cm.jnt_names[j] != FREE_JOINT:
                    foreign[b] = True
            elif t == scan_kin.BALL and not foreign[b]:
                raise NotImplementedError(f"joint {cm.jnt_names[j]!r}: ball joints are not posed")
    xpos, xquat = scan_kin.body_poses(cm, rest)
    body_link = np.zeros(cm.nbody, np.int32)      # the last link on the body or above it; 0 = base
    joints, parent, frames = [], [], []
    for b in range(1, cm.nbody):
        body_link[b] = body_link[int(cm.body_parentid[b])]
        if foreign[b]:
            body_link[b] = 0
            continue
        for j in range(int(cm.body_jntadr[b]), int(cm.body_jntadr[b]) + int(cm.body_jntnum[b])):
            if int(cm.jnt_type[j]) not in (scan_kin.SLIDE, scan_kin.HINGE):
                continue
            parent.append(int(body_link[b]) - 1)
            joints.append(j)
            frames.append((xquat[b], xpos[b] + quat2mat(xquat[b]) @ cm.jnt_pos[j]))
            body_link[b] = len(joints)
    n = len(joints)
    kin_tf, joint_tf = np.zeros((n, 7)), np.zeros((n, 6))
    for i, j in enumerate(joints):
        q, p = frames[i]
        if parent[i] >= 0:
            qp, pp = frames[parent[i]]
            qc = quat_conj(qp)
            q, p = quat_mul(qc, q), quat2mat(qc) @ (p - pp)
        kin_tf[i, :4], kin_tf[i, 4:] = _unit(q), p
        slot = 0 if int(cm.jnt_type[j]) == scan_kin.SLIDE else 3
        joint_tf[i, slot:slot + 3] = cm.jnt_axis[j]
    adr = np.array([int(cm.jnt_qposadr[j]) for j in joints], np.int64)
    return KinematicTree(parent=parent, kin_tf=kin_tf, joint_tf=joint_tf,
                         joint_names=[cm.jnt_names[j] for j in joints], theta_scan=qpos[adr] - cm.qpos0[adr],
                         qposadr=adr, qpos0=cm.qpos0[adr].copy(), body_link=body_link)
