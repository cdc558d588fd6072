"""The scan camera's matrices (reference: MjScanEnv, mgs/env/base.py:44-59,
:114-116), shared by the scan envs.  ClutterTableEnv computes the same numbers
in place."""
import numpy as np

FOVY = 45.0   # MuJoCo's default camera field of view (degrees)


def extrinsics(pos, frame) -> np.ndarray:
    """camera -> world with OpenCV axes (x right, y down, z forward): MuJoCo's
    camera frame [x, y, z | pos] turned by 180 degrees about x"""
    E = np.eye(4)
    E[:3, 0], E[:3, 1], E[:3, 2], E[:3, 3] = frame[:, 0], -frame[:, 1], -frame[:, 2], pos
    return E


def reference_intrinsics(w, h, fovy=FOVY) -> np.ndarray:
    """the reference's matrix, quirk included: fy is the pinhole focal length
    of fovy, fx that of a horizontal angle computed from fovy / 2"""
    fy = (h / 2) / np.tan(fovy * np.pi / 360)
    fx = (w / 2) / (w * 0.5 / (h * 0.5 / np.tan(fovy * np.pi / 720)))
    return np.array([[fx, 0, w / 2], [0, fy, h / 2], [0, 0, 1]])


def render_intrinsics(w, h, fovy=FOVY) -> np.ndarray:
    """what the images are rendered with: square pixels, f = fy on both axes"""
    f = (h / 2) / np.tan(fovy * np.pi / 360)
    return np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
