"""Threaded bounding-volume hierarchy of a triangle mesh, built in numpy.

Binary, median split on the longest axis of the centroid bounds, leaves of at
most LEAF_MAX triangles, nodes stored in depth-first order: node i + 1 is the
first child of an inner node i, and skip[i] is the node to visit when box i is
missed or its subtree is done (the node count at the end of the tree).  A walk
therefore needs no stack and has one fixed order (mgs_scan_kernel,
csrc/mgs_scan.hip; tests/scan_truth.py restates it).

Node boxes are padded outwards by 1e-9 x (largest side of the mesh's bounding
box) + 1e-12, far above the rounding of the slab test and of the hit points the
triangle test accepts, so pruning by a box never drops a triangle the
brute-force sweep would have hit: the rendered image equals the sweep's.
"""
from __future__ import annotations

import numpy as np

LEAF_MAX = 4


class MeshBVH:
    """box (nnode, 6: min xyz, max xyz), skip / first / count (nnode; count 0 =
    inner node, else the leaf's triangles first .. first + count - 1 of `tri`),
    tri (ntri, 9: v0 v1 v2 in BVH order), face (ntri: index into the mesh's
    own face list)."""

    def __init__(self, box, skip, first, count, tri, face, pad):
        self.box, self.skip, self.first, self.count = box, skip, first, count
        self.tri, self.face, self.pad = tri, face, pad

    @property
    def nnode(self):
        return len(self.skip)

    @property
    def ntri(self):
        return len(self.face)


def build_bvh(verts, faces) -> MeshBVH:
    v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return MeshBVH(np.zeros((0, 6)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                       np.zeros((0, 9)), np.zeros(0, np.int32), 0.0)
    tri = v[f]                                      # (nf, 3, 3)
    cen = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3.0
    tmin, tmax = tri.min(axis=1), tri.max(axis=1)
    used = v[np.unique(f)]
    pad = 1e-9 * float(np.max(used.max(axis=0) - used.min(axis=0))) + 1e-12
    box, skip, first, count, order = [], [], [], [], []

    def node(idx):
        i = len(skip)
        box.append(np.concatenate([tmin[idx].min(axis=0) - pad, tmax[idx].max(axis=0) + pad]))
        skip.append(-1)
        if len(idx) <= LEAF_MAX:
            first.append(len(order))
            count.append(len(idx))
            order.extend(int(k) for k in idx)
        else:
            first.append(0)
            count.append(0)
            c = cen[idx]
            axis = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
            by = idx[np.argsort(c[:, axis], kind="stable")]
            half = len(by) // 2
            node(by[:half])
            node(by[half:])
        skip[i] = len(skip)

    node(np.arange(len(f)))
    order = np.asarray(order, np.int64)
    return MeshBVH(np.ascontiguousarray(box, np.float64), np.asarray(skip, np.int32), np.asarray(first, np.int32),
                   np.asarray(count, np.int32), np.ascontiguousarray(tri[order].reshape(-1, 9)),
                   order.astype(np.int32), pad)
