"""Host forward kinematics of a compiled model: world poses of bodies and
geoms at a joint state, for drawing a gripper (mgs/env/gripper_scan.py).

MuJoCo's mj_kinematics restated in numpy (there is no MuJoCo in this build, so
parity with it is unpinned; at qpos0 the result is CompiledModel.body_xpos0 /
body_xquat0).  Per body, in tree order: a free joint's body sits at its qpos
(quaternion normalised); any other body starts from parent * (body_pos,
body_quat) and applies its joints in order -- a slide moves the body by
(qpos - qpos0) along the joint axis, a hinge turns it by (qpos - qpos0) about
the axis through the joint's anchor, so the anchor stays where it was.  Ball
joints are not used by any gripper here and raise.
"""
from __future__ import annotations

import numpy as np

from mgs.core.mjcf import _normq, quat2mat, quat_mul

FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3


def body_poses(cm, qpos):
    """(xpos (nbody, 3), xquat (nbody, 4) wxyz) of every body at `qpos`"""
    qpos = np.asarray(qpos, np.float64).reshape(-1)
    if qpos.shape != (cm.nq,):
        raise ValueError(f"qpos has {qpos.shape[0]} entries, the model has nq = {cm.nq}")
    xpos, xquat = np.zeros((cm.nbody, 3)), np.zeros((cm.nbody, 4))
    xquat[0] = [1.0, 0.0, 0.0, 0.0]
    for b in range(1, cm.nbody):
        p = int(cm.body_parentid[b])
        j0, nj = int(cm.body_jntadr[b]), int(cm.body_jntnum[b])
        if nj == 1 and int(cm.jnt_type[j0]) == FREE:
            a = int(cm.jnt_qposadr[j0])
            xpos[b], xquat[b] = qpos[a:a + 3], _normq(qpos[a + 3:a + 7])
            continue
        pos = xpos[p] + quat2mat(xquat[p]) @ cm.body_pos[b]
        quat = quat_mul(xquat[p], cm.body_quat[b])
        for j in range(j0, j0 + nj):
            t, a = int(cm.jnt_type[j]), int(cm.jnt_qposadr[j])
            if t not in (SLIDE, HINGE):
                raise NotImplementedError(f"joint {cm.jnt_names[j]!r}: only free (alone on its body), slide and "
                                          "hinge joints are posed")
            R = quat2mat(quat)
            anchor, axis = pos + R @ cm.jnt_pos[j], R @ cm.jnt_axis[j]
            dq = qpos[a] - cm.qpos0[a]
            if t == SLIDE:
                pos = pos + axis * dq
            else:
                ax = cm.jnt_axis[j]
                quat = quat_mul(quat, np.concatenate([[np.cos(0.5 * dq)], np.sin(0.5 * dq) * ax]))
                pos = anchor - quat2mat(quat) @ cm.jnt_pos[j]
        xpos[b], xquat[b] = pos, _normq(quat)
    return xpos, xquat


def geom_poses(cm, qpos):
    """(pos (ngeom, 3), rot (ngeom, 3, 3) frame -> world) of every compiled geom"""
    xpos, xquat = body_poses(cm, qpos)
    ng = len(cm.geom_bodyid)
    gpos, grot = np.zeros((ng, 3)), np.zeros((ng, 3, 3))
    for g in range(ng):
        b = int(cm.geom_bodyid[g])
        R = quat2mat(xquat[b])
        gpos[g] = xpos[b] + R @ cm.geom_pos[g]
        grot[g] = R @ quat2mat(_normq(cm.geom_quat[g]))
    return gpos, grot


def moved_bodies(cm, joint_name):
    """the joint's body and its descendants (ascending ids)"""
    if joint_name not in cm.jnt_names:
        raise ValueError(f"unknown joint {joint_name!r}")
    root = int(cm.jnt_bodyid[cm.jnt_names.index(joint_name)])
    moved = {root}
    for b in range(root + 1, cm.nbody):      # parents come before children
        if int(cm.body_parentid[b]) in moved:
            moved.add(b)
    return np.array(sorted(moved), np.int64)


def moved_geoms(cm, joint_name):
    """indices of the geoms the joint moves: those of its body and of every
    body below it in the tree"""
    return np.nonzero(np.isin(cm.geom_bodyid, moved_bodies(cm, joint_name)))[0]
