"""Scan scene: the drawables a ray caster sees and the arrays mgs_scan_render
takes (include/mgs_gpu.h, mgs_scan_scene).

Drawables are boxes, spheres, capsules and capped cylinders (pose, size) and
mesh instances (pose, mesh).
Meshes are instanced: two drawables with the same `key` share one BVH
(mgs/scan/bvh.py).  A drawable's index in the list is its rank in the
nearest-hit order (t, drawable index, face id); its `seg_id` is what the
segmentation image reports for it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from mgs.core import abi
from mgs.scan.bvh import MeshBVH, build_bvh

BOX, SPHERE, MESH = abi.MGS["MGS_SCAN_BOX"], abi.MGS["MGS_SCAN_SPHERE"], abi.MGS["MGS_SCAN_MESH"]
CAPSULE, CYLINDER = abi.MGS["MGS_SCAN_CAPSULE"], abi.MGS["MGS_SCAN_CYLINDER"]

# the reference's crop of the pile (render_scene_processed.py:49-53), lo xyz, hi xyz
REGION = np.array([-0.25, -0.25, -0.01, 0.25, 0.25, 1.0])


def quat_to_mat(q):
    """rotation matrix of a unit quaternion (w, x, y, z)"""
    w, x, y, z = (float(a) for a in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class ScanScene:
    def __init__(self):
        self.type, self.seg_id, self.mesh, self.pos, self.rot, self.size = [], [], [], [], [], []
        self.meshes: list[MeshBVH] = []
        self._mesh_index = {}

    def _add(self, kind, seg_id, pos, rot, size, mesh=-1):
        self.type.append(kind)
        self.seg_id.append(int(seg_id))
        self.mesh.append(int(mesh))
        self.pos.append(np.asarray(pos, np.float64).reshape(3))
        self.rot.append(np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3))
        self.size.append(np.asarray(size, np.float64).reshape(3))
        return len(self.type) - 1

    def add_box(self, seg_id, pos, rot, half_extents):
        return self._add(BOX, seg_id, pos, rot, half_extents)

    def add_sphere(self, seg_id, pos, radius):
        return self._add(SPHERE, seg_id, pos, None, [radius, 0.0, 0.0])

    def add_capsule(self, seg_id, pos, rot, radius, half_length):
        """a capsule about the frame's z: the segment (0, 0, +-half_length) swept
        by a ball of `radius`"""
        return self._add(CAPSULE, seg_id, pos, rot, [radius, half_length, 0.0])

    def add_cylinder(self, seg_id, pos, rot, radius, half_length):
        """a capped cylinder about the frame's z"""
        return self._add(CYLINDER, seg_id, pos, rot, [radius, half_length, 0.0])

    def add_mesh(self, seg_id, pos, rot, verts=None, faces=None, key=None):
        """a mesh instance; `key` names the mesh (instances of one key share its
        BVH, and only the first needs verts / faces)"""
        m = None if key is None else self._mesh_index.get(key)
        if m is None:
            if verts is None:
                raise ValueError(f"mesh {key!r} has not been added with its vertices yet")
            self.meshes.append(build_bvh(verts, faces))
            m = len(self.meshes) - 1
            if key is not None:
                self._mesh_index[key] = m
        return self._add(MESH, seg_id, pos, rot, [0.0, 0.0, 0.0], m)

    @property
    def ndraw(self):
        return len(self.type)

    def arrays(self) -> dict:
        """contiguous arrays in the field order of mgs_scan_scene"""
        i32, f64 = np.int32, np.float64
        nd = self.ndraw

        def cat(parts, shape, dt):
            return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(shape, dt), dt)
        ms = self.meshes
        return dict(
            draw_type=np.asarray(self.type, i32), draw_id=np.asarray(self.seg_id, i32),
            draw_mesh=np.asarray(self.mesh, i32),
            draw_pos=np.ascontiguousarray(self.pos, f64).reshape(nd, 3),
            draw_rot=np.ascontiguousarray(self.rot, f64).reshape(nd, 3, 3),
            draw_size=np.ascontiguousarray(self.size, f64).reshape(nd, 3),
            mesh_node0=np.concatenate([[0], np.cumsum([m.nnode for m in ms])]).astype(i32),
            mesh_tri0=np.concatenate([[0], np.cumsum([m.ntri for m in ms])]).astype(i32),
            node_box=cat([m.box for m in ms], (0, 6), f64), node_skip=cat([m.skip for m in ms], (0,), i32),
            node_first=cat([m.first for m in ms], (0,), i32), node_count=cat([m.count for m in ms], (0,), i32),
            tri=cat([m.tri for m in ms], (0, 9), f64), tri_face=cat([m.face for m in ms], (0,), i32))


def pack_scene(arrays: dict):
    """(mgs_scan_scene, the arrays it points into: keep them alive for the call)"""
    a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    s = abi.ScanScene()
    s.ndraw, s.nmesh = len(a["draw_type"]), len(a["mesh_node0"]) - 1
    s.nnode, s.ntri = len(a["node_skip"]), len(a["tri_face"])
    for name, ct in abi.ScanScene._fields_:
        if name in a:
            want = np.float64 if ct._type_ is ctypes.c_double else np.int32
            if a[name].dtype != want:
                a[name] = np.ascontiguousarray(a[name], want)
            setattr(s, name, a[name].ctypes.data_as(ct))
    return s, a


def erode_mask(mask, iterations=5):
    """binary erosion of (..., H, W) masks by a 3 x 3 square, `iterations` times,
    pixels outside the image counted as set (cv2.erode's default border, the
    reference's image mask, mgs/env/base.py:119-122)"""
    m = np.asarray(mask, bool)
    for _ in range(int(iterations)):
        p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], constant_values=True)
        h, w = m.shape[-2:]
        out = np.ones_like(m)
        for dr in range(3):
            for dc in range(3):
                out &= p[..., dr:dr + h, dc:dc + w]
        m = out
    return m


def look_at_frame(pos, target):
    """MuJoCo's `targetbody` camera frame, restated: z points from the target to
    the camera, x = (0, 0, 1) x z normalised (horizontal), y = z x x; columns
    x, y, z.  A camera straight above or below the target has no horizontal
    axis by this rule; x = (1, 0, 0) is taken there."""
    z = np.asarray(pos, np.float64) - np.asarray(target, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    n = np.linalg.norm(x)
    x = x / n if n > 1e-12 else np.array([1.0, 0.0, 0.0])
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1)
