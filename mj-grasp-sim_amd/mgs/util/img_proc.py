"""Host point-cloud processing (reference: mgs/util/img_proc.py:5-62), numpy."""
from typing import Tuple

import numpy as np


def rgbd_to_pcd(rgbd, intrinsics, extrinsics) -> Tuple[np.ndarray, np.ndarray]:
    """rgbd (N, H, W, k) with the depth last, intrinsics (3, 3), extrinsics
    (N, 4, 4) camera -> world: (points (N, H, W, 3), features (N, H, W, k - 1)).
    Pixel (row r, column c) with depth z is ((c - cx) z / fx, (r - cy) z / fy, z)
    in the camera frame -- integer pixel coordinates, no half-pixel offset, as
    the reference."""
    rgbd = np.asarray(rgbd)
    n, h, w = rgbd.shape[:3]
    fx, fy, cx, cy = intrinsics[0, 0], intrinsics[1, 1], intrinsics[0, 2], intrinsics[1, 2]
    z = rgbd[..., -1]
    x = z * (np.arange(w) - cx)[None, None, :] / fx
    y = z * (np.arange(h) - cy)[None, :, None] / fy
    cam = np.stack([x, y, z, np.ones_like(x)], axis=-1)
    world = np.einsum("nij,nhwj->nhwi", np.asarray(extrinsics, np.float64), cam)
    return world[..., :3], rgbd[..., :-1]


def voxel_downsample_pcd(points: np.ndarray, features: np.ndarray, voxel_size: float) -> Tuple[np.ndarray, np.ndarray]:
    """one point per occupied voxel of a grid anchored at the cloud's minimum
    corner: the mean position and mean feature of the voxel's points, voxels in
    ascending order of their raveled (x, y, z) grid index."""
    points = np.asarray(points)
    features = np.asarray(features)
    if len(points) == 0:
        return points.copy(), features.copy()
    cell = np.floor_divide(points - points.min(axis=0), voxel_size).astype(np.int64)
    flat = np.ravel_multi_index(cell.T, cell.max(axis=0) + 1)
    vox, inverse, count = np.unique(flat, return_inverse=True, return_counts=True)
    psum = np.zeros((len(vox), points.shape[1]), points.dtype)
    fsum = np.zeros((len(vox), features.shape[1]), features.dtype)
    np.add.at(psum, inverse, points)
    np.add.at(fsum, inverse, features)
    psum /= count[:, None]      # in place: the inputs' dtypes are kept, as the reference
    fsum /= count[:, None]
    return psum, fsum
