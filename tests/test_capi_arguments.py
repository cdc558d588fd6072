"""The C-ABI's argument checks, pinned without a GPU: every exported entry
refuses a bad call before its first HIP call, with its return code and with
its own name in mgs_last_error().  One table of bad calls at the smallest
shapes that reach each check: one view of 4 x 4 pixels, a four-triangle mesh,
three points.  (The GPU suites hold the bad-argument tests that need a device.)"""
import ctypes
import types

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    from mgs.core.engine import load_library
    return load_library()


@pytest.fixture(scope="module")
def c():
    """the valid arguments the rows start from"""
    from mgs.core import abi
    from mgs.scan.scene import ScanScene, pack_scene
    c = types.SimpleNamespace()
    c.keep = []

    def arr(a, dt=np.float64):
        a = np.ascontiguousarray(a, dt)
        c.keep.append(a)
        ct = {np.float64: ctypes.c_double, np.float32: ctypes.c_float, np.int32: ctypes.c_int32,
              np.uint8: ctypes.c_uint8, np.int64: ctypes.c_int64}[dt]
        return a.ctypes.data_as(ctypes.POINTER(ct))
    c.arr = arr
    # a tetrahedron (four triangles) and a capsule, seen by one camera of 4 x 4 pixels
    verts = np.array([[0.0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]])
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    sc = ScanScene()
    sc.add_mesh(0, [0, 0, 0.5], None, verts, faces)
    sc.add_capsule(0, [0.2, 0, 0.5], None, 0.02, 0.05)
    good = sc.arrays()

    def scene(**change):
        s, keep = pack_scene(dict(good, **{k: v.copy() for k, v in change.items()}))
        c.keep.append((s, keep))
        return ctypes.byref(s)
    c.scene = scene()
    skip = good["node_skip"].copy()
    skip[0] = 0                                  # the root's skip index points at itself: not forward
    c.scene_skip = scene(node_skip=skip)
    size = good["draw_size"].copy()
    size[1, 0] = NAN                             # the capsule's radius
    c.scene_nan = scene(draw_size=size)
    c.cam_pos, c.cam_rot, c.extr = arr(np.zeros(3)), arr(np.eye(3)), arr(np.eye(4))
    c.depth, c.seg, c.tri = arr(np.ones(16)), arr(np.zeros(16), np.int32), arr(np.zeros(16), np.int32)
    c.pts16, c.keep16 = arr(np.zeros(48)), arr(np.zeros(16), np.uint8)
    # three points
    c.p3, c.p3_nan, c.p3_inf = (arr(np.array([[0.0, 0, 0], [0.1, 0, 0], [0, x, 0]])) for x in (0.1, NAN, INF))
    c.d3, c.d9, c.i3, c.i1 = arr(np.zeros(3)), arr(np.zeros(9)), arr(np.zeros(3), np.int32), arr(np.zeros(1), np.int32)
    c.f9, c.color = arr(np.zeros(9), np.float32), arr(np.ones(3), np.float32)
    c.d64 = arr(np.zeros(64))
    c.sched = abi.Schedule()
    c.sched.nphase = 1
    c.sched = ctypes.byref(c.sched)
    c.out = ctypes.byref(abi.RolloutOut())
    c.kin = ctypes.byref(abi.KinDesc())
    c.desc = ctypes.byref(abi.ModelDesc())
    c.handle = ctypes.byref(ctypes.c_void_p())
    c.i64, c.i32 = ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int32())
    c.cint, c.u64 = ctypes.byref(ctypes.c_int()), (ctypes.c_uint64 * 2)()
    return c


def render(c, scene="scene", nview=1, w=4, h=4, fx=5.0, fy=5.0, cam_pos="cam_pos"):
    return (0, scene and getattr(c, scene), nview, cam_pos and getattr(c, cam_pos), c.cam_rot, w, h, fx, fy, 2.0, 2.0,
            c.depth, c.seg, c.tri, None, None)


def points(c, nview=1, w=4, h=4, fx=5.0, fy=5.0, erode=1, depth="depth"):
    return (0, nview, w, h, depth and getattr(c, depth), c.seg, c.extr, fx, fy, 2.0, 2.0, erode, None, c.pts16,
            c.keep16, None)


def voxels(c, n=3, pts="p3", voxel=0.01, cap=3, nfeat=0, out_nvox="i32"):
    return (0, n, getattr(c, pts), None, nfeat, None, voxel, cap, c.d9, None, None, out_nvox and getattr(c, out_nvox),
            None)


def fps(c, pts="p3", n=3, k=2, bucket=0.05):
    return (0, pts and getattr(c, pts), n, k, bucket, c.i3, None, None)


def cloud(c, scene="scene", nview=1, w=4, h=4, fx=5.0, pfx=5.0, erode=1, ncolor=1, voxel=0.01, num_points=3,
          out_n="i32"):
    return (0, scene and getattr(c, scene), nview, c.cam_pos, c.cam_rot, w, h, fx, 5.0, 2.0, 2.0, c.extr, pfx, 5.0,
            2.0, 2.0, erode, None, c.color if ncolor else None, ncolor, voxel, num_points, c.f9, c.f9,
            out_n and getattr(c, out_n), None, None)


def antipodal(c, ntri=1, n=3, tri="d9"):
    return (0, tri and getattr(c, tri), ntri, n, c.d9, c.d9, c.d3, 1e-6, c.d9, c.i3, None)


EINVAL, OK = "MGS_EINVAL", "MGS_OK"
# (entry, its arguments from the fixture, return code); a refusal names its entry
TABLE = {
    # null handles
    "model_create-null-desc": ("mgs_model_create", lambda c: (None, c.i3, c.d3, 0, c.handle), EINVAL),
    "model_create-null-out": ("mgs_model_create", lambda c: (c.desc, c.i3, c.d3, 0, None), EINVAL),
    "model_lds_bytes-null": ("mgs_model_lds_bytes", lambda c: (None, c.i64), EINVAL),
    "model_layout-null": ("mgs_model_layout", lambda c: (None, c.i3, 3, c.i32), EINVAL),
    "model_attach_special-null": ("mgs_model_attach_special", lambda c: (None, b"x.co"), EINVAL),
    "model_resident-null": ("mgs_model_resident", lambda c: (None,), EINVAL),
    "batch_open-null-model": ("mgs_batch_open", lambda c: (None, 4, c.handle), EINVAL),
    "collision_free-null-batch": ("mgs_collision_free", lambda c: (None, 1, c.d9, c.d3, c.d9, 0, None), EINVAL),
    "collision_free_device-null-batch": ("mgs_collision_free_device",
                                         lambda c: (None, 1, None, None, None, 0, None, None), EINVAL),
    "collision_free_device-negative-n": ("mgs_collision_free_device",
                                         lambda c: (None, -1, None, None, None, 0, None, None), EINVAL),
    "rollout-null-batch": ("mgs_rollout", lambda c: (None, c.sched, 1, c.d9, c.d9, c.d3, c.d3, c.out), EINVAL),
    "rollout_device-null-batch": ("mgs_rollout_device", lambda c: (None, c.sched, 1) + (None,) * 10, EINVAL),
    "simulate-null-batch": ("mgs_simulate", lambda c: (None, c.sched, 1, c.d9, None, c.d9, c.d3, c.d3, c.d64, None),
                            EINVAL),
    "simulate_device-null-batch": ("mgs_simulate_device", lambda c: (None, c.sched, 1) + (None,) * 8, EINVAL),
    "queue_stats-null-batch": ("mgs_queue_stats", lambda c: (None, c.u64), EINVAL),
    "queue_spans-null-batch": ("mgs_queue_spans", lambda c: (None, c.d64, 64, c.cint, None), EINVAL),
    "rollout_grid-null-batch": ("mgs_rollout_grid", lambda c: (None, 4), EINVAL),
    # the rollout entries' own requirements
    "rollout_resume-no-records": ("mgs_rollout_resume",
                                  lambda c: (None, c.sched, 1, c.d9, c.d9, c.d3, c.d3, None, c.out), EINVAL),
    "rollout_list_device-grid-0": ("mgs_rollout_list_device",
                                   lambda c: (None, c.sched, 1, None, None, 0) + (None,) * 10, EINVAL),
    "rollout_resumable_device-no-resume-buffer": ("mgs_rollout_resumable_device",
                                                  lambda c: (None, c.sched, 1) + (None,) * 12, EINVAL),
    "mask_rollout_device-no-free_out": ("mgs_mask_rollout_device",
                                        lambda c: (None, c.sched, 1, None, ctypes.cast(c.d3, ctypes.c_void_p), None,
                                                   None, None, 0) + (None,) * 8, EINVAL),
    "overflow_list_device-negative-n": ("mgs_overflow_list_device", lambda c: (-1, None, 3, None, None, None), EINVAL),
    # negative sizes and null arrays of the one-shot entries
    "antipodal-negative-n": ("mgs_antipodal_contacts", lambda c: antipodal(c, n=-1), EINVAL),
    "antipodal-negative-ntri": ("mgs_antipodal_contacts", lambda c: antipodal(c, ntri=-1), EINVAL),
    "antipodal-null-tri": ("mgs_antipodal_contacts", lambda c: antipodal(c, tri=None), EINVAL),
    "arith_probe-negative-n": ("mgs_arith_probe", lambda c: (c.d3, c.d3, -1, c.d64), EINVAL),
    "arith_probe-null-input": ("mgs_arith_probe", lambda c: (None, c.d3, 3, c.d64), EINVAL),
    "arith_probe-nothing": ("mgs_arith_probe", lambda c: (None, None, 0, None), OK),
    "tree_probe-negative-n": ("mgs_tree_probe", lambda c: (c.d64, c.d64, -1, 1, c.d3), EINVAL),
    "tree_probe-negative-nb": ("mgs_tree_probe", lambda c: (c.d64, c.d64, 3, -1, c.d3), EINVAL),
    "tree_probe-null-input": ("mgs_tree_probe", lambda c: (None, c.d64, 3, 1, c.d3), EINVAL),
    "tree_probe-nothing": ("mgs_tree_probe", lambda c: (None, None, 3, 0, None), OK),
    "contact_fps-k-above-n": ("mgs_contact_fps", lambda c: (0, c.p3, 3, 4, c.i3, None), EINVAL),
    "contact_fps-negative-n": ("mgs_contact_fps", lambda c: (0, c.p3, -1, 0, c.i3, None), EINVAL),
    "contact_fps-null-points": ("mgs_contact_fps", lambda c: (0, None, 3, 2, c.i3, None), EINVAL),
    "contact_seeds-negative-k": ("mgs_contact_seeds", lambda c: (0, c.p3, -1, 0.1, 0, 1, c.i3, c.i3, None), EINVAL),
    "contact_seeds-no-tip": ("mgs_contact_seeds", lambda c: (0, c.p3, 3, 0.1, 0, 0, c.i3, c.i3, None), EINVAL),
    "contact_seeds-null-seeds": ("mgs_contact_seeds", lambda c: (0, None, 3, 0.1, 0, 1, c.i3, c.i3, None), EINVAL),
    "contact_optimize-null-kin": ("mgs_contact_optimize", lambda c: (0, None, 1) + (c.d9,) * 8 + (None,), EINVAL),
    "contact_optimize-negative-n": ("mgs_contact_optimize", lambda c: (0, c.kin, -1) + (c.d9,) * 8 + (None,), EINVAL),
    # the scan entries: views, focal lengths, erosion, the scene's indices and sizes
    "scan_render-null-scene": ("mgs_scan_render", lambda c: render(c, scene=None), EINVAL),
    "scan_render-negative-views": ("mgs_scan_render", lambda c: render(c, nview=-1), EINVAL),
    "scan_render-negative-width": ("mgs_scan_render", lambda c: render(c, w=-4), EINVAL),
    "scan_render-negative-height": ("mgs_scan_render", lambda c: render(c, h=-4), EINVAL),
    "scan_render-too-many-views": ("mgs_scan_render", lambda c: render(c, nview=65536, w=1, h=1), EINVAL),
    "scan_render-too-many-pixels": ("mgs_scan_render", lambda c: render(c, nview=2, w=32768, h=32768), EINVAL),
    "scan_render-focal-0": ("mgs_scan_render", lambda c: render(c, fx=0.0), EINVAL),
    "scan_render-focal-negative": ("mgs_scan_render", lambda c: render(c, fy=-5.0), EINVAL),
    "scan_render-focal-nan": ("mgs_scan_render", lambda c: render(c, fx=NAN), EINVAL),
    "scan_render-backward-skip": ("mgs_scan_render", lambda c: render(c, scene="scene_skip"), EINVAL),
    "scan_render-capsule-radius-nan": ("mgs_scan_render", lambda c: render(c, scene="scene_nan"), EINVAL),
    "scan_render-null-camera": ("mgs_scan_render", lambda c: render(c, cam_pos=None), EINVAL),
    "scan_points-negative-views": ("mgs_scan_points", lambda c: points(c, nview=-1), EINVAL),
    "scan_points-negative-width": ("mgs_scan_points", lambda c: points(c, w=-4), EINVAL),
    "scan_points-too-many-pixels": ("mgs_scan_points", lambda c: points(c, nview=2, w=32768, h=32768), EINVAL),
    "scan_points-focal-0": ("mgs_scan_points", lambda c: points(c, fy=0.0), EINVAL),
    "scan_points-focal-negative": ("mgs_scan_points", lambda c: points(c, fx=-1.0), EINVAL),
    "scan_points-erode-negative": ("mgs_scan_points", lambda c: points(c, erode=-1), EINVAL),
    "scan_points-erode-65": ("mgs_scan_points", lambda c: points(c, erode=65), EINVAL),
    "scan_points-null-depth": ("mgs_scan_points", lambda c: points(c, depth=None), EINVAL),
    "scan_voxels-negative-n": ("mgs_scan_voxels", lambda c: voxels(c, n=-1), EINVAL),
    "scan_voxels-negative-cap": ("mgs_scan_voxels", lambda c: voxels(c, cap=-1), EINVAL),
    "scan_voxels-voxel-0": ("mgs_scan_voxels", lambda c: voxels(c, voxel=0.0), EINVAL),
    "scan_voxels-voxel-inf": ("mgs_scan_voxels", lambda c: voxels(c, voxel=INF), EINVAL),
    "scan_voxels-voxel-nan": ("mgs_scan_voxels", lambda c: voxels(c, voxel=NAN), EINVAL),
    "scan_voxels-point-nan": ("mgs_scan_voxels", lambda c: voxels(c, pts="p3_nan"), EINVAL),
    "scan_voxels-point-inf": ("mgs_scan_voxels", lambda c: voxels(c, pts="p3_inf"), EINVAL),
    "scan_voxels-null-out_nvox": ("mgs_scan_voxels", lambda c: voxels(c, out_nvox=None), EINVAL),
    "scan_fps-k-above-n": ("mgs_scan_fps", lambda c: fps(c, k=4), EINVAL),
    "scan_fps-negative-n": ("mgs_scan_fps", lambda c: fps(c, n=-1, k=0), EINVAL),
    "scan_fps-bucket-0": ("mgs_scan_fps", lambda c: fps(c, bucket=0.0), EINVAL),
    "scan_fps-bucket-nan": ("mgs_scan_fps", lambda c: fps(c, bucket=NAN), EINVAL),
    "scan_fps-bucket-inf": ("mgs_scan_fps", lambda c: fps(c, bucket=INF), EINVAL),
    "scan_fps-point-nan": ("mgs_scan_fps", lambda c: fps(c, pts="p3_nan"), EINVAL),
    "scan_fps-point-inf": ("mgs_scan_fps", lambda c: fps(c, pts="p3_inf"), EINVAL),
    "scan_fps-null-points": ("mgs_scan_fps", lambda c: fps(c, pts=None), EINVAL),
    "scan_cloud-null-scene": ("mgs_scan_cloud", lambda c: cloud(c, scene=None), EINVAL),
    "scan_cloud-negative-views": ("mgs_scan_cloud", lambda c: cloud(c, nview=-1), EINVAL),
    "scan_cloud-negative-num_points": ("mgs_scan_cloud", lambda c: cloud(c, num_points=-1), EINVAL),
    "scan_cloud-too-many-views": ("mgs_scan_cloud", lambda c: cloud(c, nview=65536, w=1, h=1), EINVAL),
    "scan_cloud-too-many-pixels": ("mgs_scan_cloud", lambda c: cloud(c, nview=2, w=32768, h=32768), EINVAL),
    "scan_cloud-focal-0": ("mgs_scan_cloud", lambda c: cloud(c, fx=0.0), EINVAL),
    "scan_cloud-points-focal-0": ("mgs_scan_cloud", lambda c: cloud(c, pfx=0.0), EINVAL),
    "scan_cloud-erode-negative": ("mgs_scan_cloud", lambda c: cloud(c, erode=-1), EINVAL),
    "scan_cloud-erode-65": ("mgs_scan_cloud", lambda c: cloud(c, erode=65), EINVAL),
    "scan_cloud-voxel-nan": ("mgs_scan_cloud", lambda c: cloud(c, voxel=NAN), EINVAL),
    "scan_cloud-voxel-inf": ("mgs_scan_cloud", lambda c: cloud(c, voxel=INF), EINVAL),
    "scan_cloud-draw_id-without-colour": ("mgs_scan_cloud", lambda c: cloud(c, ncolor=0), EINVAL),
    "scan_cloud-backward-skip": ("mgs_scan_cloud", lambda c: cloud(c, scene="scene_skip"), EINVAL),
    "scan_cloud-capsule-radius-nan": ("mgs_scan_cloud", lambda c: cloud(c, scene="scene_nan"), EINVAL),
    "scan_cloud-null-out_n": ("mgs_scan_cloud", lambda c: cloud(c, out_n=None), EINVAL),
}


@pytest.mark.parametrize("row", sorted(TABLE))
def test_bad_call_is_refused_by_name(L, c, row):
    from mgs.core import abi
    entry, args, code = TABLE[row]
    fn = getattr(L, entry)
    fn.restype = ctypes.c_int
    assert fn(*args(c)) == abi.MGS[code]
    if code != OK:
        assert entry.encode() in L.mgs_last_error(), L.mgs_last_error()
