"""Scene cloud on the MI355X (csrc/mgs_cloud.hip through the C-ABI): the voxel
grid against the host function and the numpy truth, the pruned farthest-point
pick against mgs_contact_fps and the truth (indices and evaluation counts), the
composition mgs_scan_cloud against the truth's, then ClutterTableEnv.scan_cloud
and the render_scene_processed CLI.  Every comparison is bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_truth as C  # noqa: E402
import scan_truth as T  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 37, 29
PD, PF = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
PI, PU8, PI64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(got_p, got_f, want_p, want_f):
    return (got_p.shape == want_p.shape and np.array_equal(bits(got_p), bits(want_p)) and got_f.dtype == np.float32
            and got_f.shape == want_f.shape and np.array_equal(bits32(got_f), bits32(want_f)))


# -- voxels -------------------------------------------------------------------
@pytest.fixture(scope="module")
def adversarial():
    return C.adversarial_cloud()


@pytest.mark.parametrize("nfeat", [3, 0])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("voxel_size", [0.002, 0.0123])
def test_voxels_adversarial(adversarial, voxel_size, masked, nfeat):
    from mgs.core.engine import scan_voxels
    from mgs.util.img_proc import voxel_downsample_pcd
    P, F, keep = adversarial
    F = F[:, :nfeat]
    k = keep if masked else None
    gp, gf, gc, ms = scan_voxels(P, F, voxel_size, keep=k)
    hp, hf = voxel_downsample_pcd(P[keep], F[keep], voxel_size) if masked else voxel_downsample_pcd(P, F, voxel_size)
    tp, tf, tc = C.voxels(P, F, voxel_size, k)
    assert same(gp, gf, hp, hf)
    assert same(gp, gf, tp, tf) and np.array_equal(gc, tc)
    assert ms > 0 and 1 < len(gp) < len(P)


@pytest.fixture(scope="module")
def small():
    """the small scan scene's truth images and points (4 views of 37 x 29)"""
    S = T.small_scene().arrays()
    pos, R = T.small_cameras()
    f = T.focal(H)
    o, d = T.camera_rays(pos, R, W, H, f, f, W / 2, H / 2)
    depth, seg, _, _ = T.render_bvh(S, o, d, (len(pos), H, W))
    E = np.tile(np.eye(4), (len(pos), 1, 1))
    E[:, :3, :3], E[:, :3, 3] = R, pos
    colors = np.random.default_rng(1).uniform(0, 1, (16, 3)).astype(np.float32)     # seg ids 10 .. 15
    return dict(S=S, pos=pos, R=R, E=E, f=f, depth=depth, seg=seg, colors=colors)


def test_voxels_small_scene(small):
    from mgs.core.engine import scan_voxels
    from mgs.util.img_proc import voxel_downsample_pcd
    P, keep = T.points(small["depth"], small["seg"], small["E"], 73.0, small["f"], W / 2, H / 2, 5)
    P, keep = P.reshape(-1, 3), keep.reshape(-1)
    F = small["colors"][np.where(small["seg"] < 0, 0, small["seg"])].reshape(-1, 3)
    assert 100 < keep.sum() < len(P)
    for vs in (0.01, 0.002):
        gp, gf, gc, _ = scan_voxels(P, F, vs, keep=keep)
        hp, hf = voxel_downsample_pcd(P[keep], F[keep], vs)
        assert same(gp, gf, hp, hf) and gc.sum() == keep.sum()
        assert same(gp, gf, *C.voxels(P, F, vs, keep)[:2])


def test_voxels_tiny_inputs():
    from mgs.core.engine import scan_voxels
    P = np.array([[0.3, -0.2, 0.1], [0.5, 0.5, 0.5]])
    F = np.array([[0.25, 0.5], [1.0, 2.0]], np.float32)
    gp, gf, gc, _ = scan_voxels(P[:1], F[:1], 0.002)
    assert np.array_equal(gp, P[:1]) and np.array_equal(gf, F[:1]) and gc.tolist() == [1]
    gp, gf, gc, _ = scan_voxels(P, F, 0.002, keep=np.array([False, True]))
    assert np.array_equal(gp, P[1:]) and np.array_equal(gf, F[1:])
    for args in ((P, F, 0.002, np.zeros(2, bool)), (P[:0], F[:0], 0.002, None)):
        gp, gf, gc, _ = scan_voxels(*args[:3], keep=args[3])
        assert gp.shape == (0, 3) and gf.shape == (0, 2) and len(gc) == 0
    # -0.0 sums to +0.0, as np.add.at from zeros
    gp, _, _, _ = scan_voxels(np.array([[-0.0, -0.0, -0.0]]), None, 0.002)
    assert np.array_equal(bits(gp), bits(np.zeros((1, 3))))


def raw_voxels(L, P, keep, F, voxel_size, cap, fill=7.0, n=None, nfeat=None):
    nfeat = F.shape[1] if nfeat is None else nfeat
    rows = max(cap, 1)
    oP, oF, oC = np.full((rows, 3), fill), np.full((rows, max(nfeat, 1)), fill, np.float32), np.full(rows, 7, np.int32)
    nv = ctypes.c_int32(-5)
    rc = L.mgs_scan_voxels(0, len(P) if n is None else n, P.ctypes.data_as(PD),
                           None if keep is None else keep.ctypes.data_as(PU8), nfeat, F.ctypes.data_as(PF),
                           voxel_size, cap, oP.ctypes.data_as(PD), oF.ctypes.data_as(PF), oC.ctypes.data_as(PI),
                           ctypes.byref(nv), None)
    return rc, nv.value, oP, oF, oC


def test_voxels_capacity_and_bad_arguments(adversarial):
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    P, F, keep = adversarial
    P, F = np.ascontiguousarray(P[:600]), np.ascontiguousarray(F[:600])
    k8 = np.ascontiguousarray(keep[:600], np.uint8)
    want = C.voxels(P, F, 0.002, keep[:600])
    nvox = len(want[0])
    untouched = lambda oP, oF, oC: np.all(oP == 7.0) and np.all(oF == 7.0) and np.all(oC == 7)      # noqa: E731
    rc, nv, oP, oF, oC = raw_voxels(L, P, k8, F, 0.002, nvox - 1)
    assert rc == abi.MGS["MGS_ECAPACITY"] and nv == nvox and untouched(oP, oF, oC)
    # a grid past MGS_CLOUD_MAX_CELLS: 3 m at 1 mm
    far = np.array([[0.0, 0.0, 0.0], [3.0, 3.0, 3.0]])
    rc, nv, oP, oF, oC = raw_voxels(L, far, None, F[:2], 0.001, 2)
    assert rc == abi.MGS["MGS_ECAPACITY"] and nv == -1 and untouched(oP, oF, oC)
    bad_point = P.copy()
    bad_point[np.nonzero(k8)[0][3], 1] = np.nan
    inf_point = P.copy()
    inf_point[np.nonzero(k8)[0][5], 2] = np.inf
    huge = np.array([[0.0, 0.0, 0.0], [1e300, 1e300, 1e300]])
    cases = [dict(P=P, vs=0.0), dict(P=P, vs=-0.002), dict(P=P, vs=np.nan), dict(P=P, vs=np.inf),
             dict(P=bad_point, vs=0.002), dict(P=inf_point, vs=0.002), dict(P=P, vs=0.002, n=-1),
             dict(P=P, vs=0.002, nfeat=-1), dict(P=P, vs=0.002, cap=-1)]
    for c in cases:
        rc, nv, oP, oF, oC = raw_voxels(L, c["P"], k8, F, c["vs"], c.get("cap", 600), n=c.get("n"), nfeat=c.get("nfeat"))
        assert rc == abi.MGS["MGS_EINVAL"], c
        assert nv == -5 and untouched(oP, oF, oC), c
        assert b"mgs_scan_voxels" in L.mgs_last_error()
    rc, nv, oP, oF, oC = raw_voxels(L, huge, None, F[:2], 1e-3, 2)            # the raveled index overflows int64
    assert rc == abi.MGS["MGS_EINVAL"] and nv == -5 and untouched(oP, oF, oC)
    # a non-finite point that is not kept is nobody's business, and a valid call works afterwards
    dropped = P.copy()
    dropped[np.nonzero(k8 == 0)[0][0]] = np.nan
    rc, nv, oP, oF, oC = raw_voxels(L, dropped, k8, F, 0.002, 600)
    assert rc == 0 and nv == nvox
    assert same(oP[:nv], oF[:nv], want[0], want[1]) and np.array_equal(oC[:nv], want[2])
    assert np.all(oP[nv:] == 7.0) and np.all(oC[nv:] == 7)


# -- the pick -----------------------------------------------------------------
def check_pick(x, k, bucket):
    from mgs.core.engine import contact_fps, scan_fps
    got, nevals, ms = scan_fps(x, k, bucket)
    want, _ = contact_fps(x, k)
    assert np.array_equal(got, want)
    tidx, tevals, _ = C.bucket_fps(x, k, bucket)
    assert np.array_equal(got, tidx) and nevals == tevals
    return nevals


@pytest.mark.parametrize("n,k", [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (1025, 200)])
def test_pick_sizes(n, k):
    x = np.random.default_rng(n).uniform(-0.1, 0.1, (n, 3)).astype(np.float32).astype(np.float64)
    nevals = check_pick(x, k, 0.016)
    assert nevals <= n * (k - 1)
    assert np.array_equal(C.brute_fps(x, k), C.bucket_fps(x, k, 0.016)[0])


@pytest.mark.parametrize("bucket", [0.016, 0.004, 1.0, 1e-5])
def test_pick_lattice_with_ties(bucket):
    x = C.lattice()
    check_pick(x, len(x), bucket)


@pytest.fixture(scope="module")
def surface():
    x = C.surface_cloud()
    return x, C.brute_fps(x, 600)


def test_pick_surface_prunes(surface):
    from mgs.core.engine import scan_fps
    x, want = surface
    n, k = len(x), 600
    got, nevals, _ = scan_fps(x, k, 0.016)
    tidx, tevals, nbucket = C.bucket_fps(x, k, 0.016)
    assert np.array_equal(got, want) and np.array_equal(tidx, want)
    assert nevals == tevals and 0 < nevals < 0.1 * n * (k - 1) and nbucket > 100


def test_pick_one_bucket_and_one_point_buckets(surface):
    from mgs.core.engine import scan_fps
    x, want = surface
    n, k = len(x), 600
    got, nevals, _ = scan_fps(x, k, 10.0)                       # one bucket: the sweep
    assert np.array_equal(got, want) and nevals == n * (k - 1)
    got, nevals, _ = scan_fps(x, k, 1e-6)                       # the side doubles to the 2^24-cell grid
    tidx, tevals, nbucket = C.bucket_fps(x, k, 1e-6)
    assert nbucket > 0.9 * n
    assert np.array_equal(got, want) and np.array_equal(tidx, want) and nevals == tevals


def test_pick_bad_arguments():
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    x = np.random.default_rng(0).uniform(0, 1, (10, 3))
    out = np.full(10, 7, np.int32)
    nev = ctypes.c_int64(-5)

    def call(pts, n, k, bucket):
        return L.mgs_scan_fps(0, None if pts is None else pts.ctypes.data_as(PD), n, k, bucket, out.ctypes.data_as(PI),
                              ctypes.byref(nev), None)
    bad = x.copy()
    bad[4, 1] = np.inf
    for args in ((x, 10, 11, 0.1), (x, -1, 0, 0.1), (x, 10, -1, 0.1), (x, 10, 5, 0.0), (x, 10, 5, -0.1), (x, 10, 5, np.nan),
                 (x, 10, 5, np.inf), (None, 10, 5, 0.1), (bad, 10, 5, 0.1)):
        assert call(*args) == abi.MGS["MGS_EINVAL"], args[1:]
        assert b"mgs_scan_fps" in L.mgs_last_error()
    assert np.all(out == 7) and nev.value == -5
    assert call(x, 10, 10, 0.1) == 0 and sorted(out.tolist()) == list(range(10)) and nev.value > 0


# -- the composition ----------------------------------------------------------
def raw_cloud(L, small, num_points, voxel_size, rows, scene=None, ncolor=16, fill=7.0):
    from mgs.scan.scene import pack_scene
    sc, keep = pack_scene(small["S"]) if scene is None else scene
    oP, oC = np.full((rows, 3), fill, np.float32), np.full((rows, 3), fill, np.float32)
    n = ctypes.c_int32(-5)
    stats, stages = np.full(8, -5, np.int64), np.full(4, -5.0)
    pos, R, E = (np.ascontiguousarray(small[k]) for k in ("pos", "R", "E"))
    f = small["f"]
    rc = L.mgs_scan_cloud(0, ctypes.byref(sc), len(pos), pos.ctypes.data_as(PD), R.ctypes.data_as(PD), W, H, f, f, W / 2,
                          H / 2, E.ctypes.data_as(PD), 73.0, f, W / 2, H / 2, 5, None, small["colors"].ctypes.data_as(PF),
                          ncolor, voxel_size, num_points, oP.ctypes.data_as(PF), oC.ctypes.data_as(PF), ctypes.byref(n),
                          stats.ctypes.data_as(PI64), stages.ctypes.data_as(PD))
    del keep
    return rc, n.value, oP, oC, stats, stages


def truth_cloud(small, num_points, voxel_size):
    f = small["f"]
    return C.cloud(small["S"], small["pos"], small["R"], W, H, f, f, W / 2, H / 2, small["E"], 73.0, f, W / 2, H / 2, 5, None,
                   small["colors"], voxel_size, num_points)


def test_cloud_small_scene(small):
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    tp, tc, info = truth_cloud(small, 64, 0.01)
    assert info["voxels"] >= 64 and len(tp) == 64 and info["evals"] > 0
    rc, n, oP, oC, stats, stages = raw_cloud(L, small, 64, 0.01, rows=80)
    assert rc == 0 and n == 64
    assert np.array_equal(bits32(oP[:64]), bits32(tp)) and np.array_equal(bits32(oC[:64]), bits32(tc))
    assert np.all(oP[64:] == 7.0) and np.all(oC[64:] == 7.0)                   # beyond out_n: untouched
    assert stats[:6].tolist() == [info["kept"], info["voxels"], info["evals"], stats[3], 64, 4 * W * H]
    assert 0 < stats[3] <= abi.MGS["MGS_CLOUD_MAX_CELLS"] and np.all(stages > 0)
    # more points asked for than there are voxels: every voxel, in voxel order
    ap, ac, ainfo = truth_cloud(small, 100000, 0.01)
    assert len(ap) == info["voxels"] and ainfo["evals"] == 0
    rc, n, oP, oC, stats, _ = raw_cloud(L, small, 1000, 0.01, rows=1000)
    assert rc == 0 and n == info["voxels"] and stats[2] == 0
    assert np.array_equal(bits32(oP[:n]), bits32(ap)) and np.array_equal(bits32(oC[:n]), bits32(ac))
    assert np.all(oP[n:] == 7.0) and np.all(oC[n:] == 7.0)
    # the wrapper
    from mgs.core.engine import scan_cloud
    f = small["f"]
    gp, gc, ginfo = scan_cloud(small["S"], small["pos"], small["R"], W, H, f, f, W / 2, H / 2, small["E"], 73.0, f, W / 2,
                               H / 2, small["colors"], 64, voxel_size=0.01)
    assert np.array_equal(bits32(gp), bits32(tp)) and np.array_equal(bits32(gc), bits32(tc))
    assert ginfo["kept"] == info["kept"] and ginfo["pick_evals"] == info["evals"] and ginfo["pick_ms"] > 0


def test_cloud_bad_arguments(small):
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    for kw in (dict(num_points=-1, voxel_size=0.01), dict(num_points=8, voxel_size=0.0),
               dict(num_points=8, voxel_size=np.nan), dict(num_points=8, voxel_size=0.01, ncolor=15)):   # draw_id 15 has no row
        rc, n, oP, oC, stats, stages = raw_cloud(L, small, rows=8, **kw)
        assert rc == abi.MGS["MGS_EINVAL"], kw
        assert b"mgs_scan_cloud" in L.mgs_last_error()
        assert n == -5 and np.all(oP == 7.0) and np.all(oC == 7.0) and np.all(stats == -5) and np.all(stages == -5.0)
    rc, n, oP, _, _, _ = raw_cloud(L, small, 8, 0.01, rows=8)
    assert rc == 0 and n == 8 and not np.any(oP == 7.0)


# -- the env and the CLI ------------------------------------------------------
@pytest.fixture(scope="module")
def cenv():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_clutter_scene import make_env
    from mgs.env.clutter_table import ClutterTableEnv
    env = make_env()
    z = np.load(os.path.join(HERE, "golden", "clutter_scene.npz"))
    return ClutterTableEnv.from_dict({"gripper": env.gripper, "objects": env.objects,
                                      "env_state": {"state": z["state"]}})


def test_env_scan_cloud_equals_the_pieces(cenv):
    from mgs.core.engine import contact_fps, scan_points
    from mgs.scan.scene import REGION
    from mgs.util.img_proc import voxel_downsample_pcd
    n, w, h, num = 3, 64, 64, 256
    P, Cl = cenv.scan_cloud(n, num_points=num, width=w, height=h)
    assert P.dtype == np.float32 and Cl.dtype == np.float32 and P.shape == Cl.shape and P.shape[1] == 3
    info = cenv.last_cloud
    rgbd, extr, masks, seg = cenv.scan(num_images=n, width=w, height=h)
    K = cenv.get_camera_intrinsics()
    depth = rgbd[..., 3].astype(np.float64)
    assert np.array_equal(rgbd[..., 3], cenv.last_scan["depth"].astype(np.float32))
    pts, keep, _ = scan_points(depth, seg, extr, K[0, 0], K[1, 1], K[0, 2], K[1, 2], erode_iters=5, region=REGION)
    feat = cenv.scan_colors().astype(np.float32)[seg[keep]]
    vp, vf = voxel_downsample_pcd(pts[keep], feat, 0.002)
    assert info["kept"] == keep.sum() and info["voxels"] == len(vp) > 0 and info["pixels"] == n * w * h
    if len(vp) >= num:
        idx, _ = contact_fps(vp.astype(np.float32), num)
        assert 0 < info["pick_evals"] <= len(vp) * (num - 1)
    else:
        idx = np.arange(len(vp))
        assert info["pick_evals"] == 0
    assert info["rows"] == len(idx) == len(P) and info["render_ms"] > 0
    assert np.array_equal(bits32(P), bits32(vp[idx].astype(np.float32)))
    assert np.array_equal(bits32(Cl), bits32(vf[idx]))


def test_render_scene_processed_cli_cloud_key(cenv, tmp_path, monkeypatch, capsys):
    from mgs.cli import render_scene_processed
    from mgs.env.selector import save_scene
    d = tmp_path / "in" / "Robotiq2f85Gripper" / "scene_000"
    d.mkdir(parents=True)
    save_scene(d / "scene.npz", cenv.to_dict())
    monkeypatch.setenv("MGS_INPUT_DIR", str(tmp_path / "in"))
    args = ["gripper=robotiq_2f_85", "id=0", "num_images=4", "width=64", "height=64", "num_points=256"]
    files = {}
    for name, extra in (("plain", []), ("host", ["cloud=host"]), ("device", ["cloud=device"]),
                        ("few", ["cloud=device", "num_points=100000"])):
        monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / name))
        capsys.readouterr()
        render_scene_processed.run(args + extra)
        files[name] = tmp_path / name / "Robotiq2f85Gripper" / "scene_000" / "scene_pcd.npz"
        printed = capsys.readouterr().out
        asked = 100000 if name == "few" else 256
        assert ("all kept" in printed) == (len(np.load(files[name])["points"]) < asked)
    assert files["plain"].read_bytes() == files["host"].read_bytes()
    lo, hi = np.float32([-0.25, -0.25, -0.01]), np.float32([0.25, 0.25, 1.0])
    for name in ("device", "few"):
        z = np.load(files[name])
        assert sorted(z.files) == sorted(np.load(files["plain"]).files) == ["colors", "points"]
        P, Cl = z["points"], z["colors"]
        assert P.dtype == np.float32 and Cl.dtype == np.float32
        assert P.ndim == 2 and P.shape[1] == 3 and Cl.shape == (len(P), 3)
        assert 0 < len(P) <= (256 if name == "device" else 100000)
        assert np.all(P >= lo) and np.all(P <= hi) and len(np.unique(P, axis=0)) == len(P)
        assert Cl.min() >= 0 and Cl.max() <= 1
