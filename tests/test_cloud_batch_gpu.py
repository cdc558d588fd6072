"""Many scene clouds per call on the MI355X (mgs_scan_fps_batch,
mgs_scan_cloud_batch: one pick workgroup per cloud): per cloud exactly what the
single-cloud entries and the numpy truth (tests/cloud_truth.py) give, whatever
the order and the number of clouds; errors found before anything is written;
then mgs.env.clutter_table.scan_clouds and the CLI's `ids` key.  Every
comparison is bit for bit: indices as int32, floats through their integer
views."""
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
VS = 0.01
PD, PF = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
PI, PI64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def random_cloud(n, seed=None):
    """the clouds of test_cloud_gpu.test_pick_sizes"""
    return np.random.default_rng(n if seed is None else seed).uniform(-0.1, 0.1, (n, 3)).astype(np.float32).astype(np.float64)


def check_batch(clouds, ks, bucket, truth):
    """one batched call; per cloud the truth's indices and evaluation count"""
    from mgs.core.engine import scan_fps_batch
    idx, nev, ms = scan_fps_batch(clouds, ks, bucket)
    assert len(idx) == len(clouds) and nev.shape == (len(clouds),) and nev.dtype == np.int64
    for c, (want, evals) in enumerate(truth):
        assert idx[c].dtype == np.int32 and idx[c].shape == (ks[c],), c
        assert np.array_equal(idx[c], want), c
        assert nev[c] == evals, c
    return idx, nev, ms


# -- the ragged pick ----------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """clouds, picks and (truth indices, truth evaluations) at bucket 0.016: the
    sizes around a wave, an empty cloud in the middle, a cloud nobody picks
    from, ties (the lattice) and pruning (the surface)"""
    sizes = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (1025, 200)]
    clouds = [random_cloud(n) for n, _ in sizes]
    ks = [k for _, k in sizes]
    clouds[3:3] = [np.zeros((0, 3)), random_cloud(50, seed=77)]
    ks[3:3] = [0, 0]
    lat, surf = C.lattice(), C.surface_cloud()
    clouds += [lat, surf]
    ks += [len(lat), 600]
    truth = []
    for x, k in zip(clouds, ks):
        idx, evals, _ = C.bucket_fps(x, k, 0.016)
        truth.append((idx, evals))
    return clouds, ks, truth


def test_ragged_pick(ragged):
    from mgs.core.engine import scan_fps
    clouds, ks, truth = ragged
    assert [len(x) for x in clouds][3:5] == [0, 50] and ks[3:5] == [0, 0]
    idx, nev, ms = check_batch(clouds, ks, 0.016, truth)
    assert ms > 0
    for c, (x, k) in enumerate(zip(clouds, ks)):
        got, evals, _ = scan_fps(x, k, 0.016)
        assert np.array_equal(idx[c], got) and nev[c] == evals, c
    assert nev[3] == 0 and nev[4] == 0 and nev[0] == 0 and nev[-1] > 0


# -- bucket sizes ---------------------------------------------------------------
@pytest.mark.parametrize("bucket", [0.016, 0.004, 1.0, 1e-5])
def test_bucket_sizes(bucket):
    """from one bucket for everything to one point per bucket; at 1e-5 the
    surface has more buckets than the LDS visit list holds (MGS_CLOUD_FPS_TILE,
    4096), so the list goes in passes inside a batch"""
    lat, surf, small = C.lattice(), C.surface_cloud(6000), random_cloud(65)
    clouds, ks = [lat, surf, small], [len(lat), 300, 65]
    truth, nbucket = [], []
    for x, k in zip(clouds, ks):
        idx, evals, nb = C.bucket_fps(x, k, bucket)
        truth.append((idx, evals))
        nbucket.append(nb)
    if bucket == 1.0:
        assert nbucket == [1, 1, 1]
    if bucket == 1e-5:
        assert nbucket[0] == 315 and nbucket[1] > 4096
    check_batch(clouds, ks, bucket, truth)


# -- order and count ----------------------------------------------------------
def test_order_of_the_clouds_changes_nothing(ragged):
    clouds, ks, truth = ragged
    n = len(clouds)
    for perm in (list(range(n))[::-1], np.random.default_rng(8).permutation(n).tolist()):
        check_batch([clouds[c] for c in perm], [ks[c] for c in perm], 0.016, [truth[c] for c in perm])


def test_more_clouds_than_resident_workgroups():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ncloud = max(600, 2 * cus + 88)              # two 1024-lane workgroups fit a CU
    rng = np.random.default_rng(21)
    clouds = [rng.uniform(-0.1, 0.1, (65, 3)).astype(np.float32).astype(np.float64) for _ in range(ncloud)]
    ks = [8] * ncloud
    truth = [C.bucket_fps(x, 8, 0.016)[:2] for x in clouds]
    check_batch(clouds, ks, 0.016, truth)


def test_batch_of_one_and_of_none(ragged):
    from mgs.core.engine import scan_fps, scan_fps_batch
    clouds, ks, truth = ragged
    idx, nev, _ = check_batch(clouds[-1:], ks[-1:], 0.016, truth[-1:])
    got, evals, _ = scan_fps(clouds[-1], ks[-1], 0.016)
    assert np.array_equal(idx[0], got) and nev[0] == evals
    idx, nev, ms = scan_fps_batch([], [], 0.016)
    assert idx == [] and len(nev) == 0 and ms == 0.0
    idx, nev, _ = scan_fps_batch([clouds[4], clouds[3]], [0, 0], 0.016)        # nothing to pick anywhere
    assert [len(i) for i in idx] == [0, 0] and nev.tolist() == [0, 0]


# -- the composition ----------------------------------------------------------
def variant(S, moved=None, removed=None):
    """the scene's arrays with drawable `moved` shifted or drawable `removed` taken out"""
    S = {k: np.array(v) for k, v in S.items()}
    if moved is not None:
        S["draw_pos"][moved] += [0.03, 0.05, 0.0]
    if removed is not None:
        for k in [k for k in S if k.startswith("draw_")]:
            S[k] = np.ascontiguousarray(np.delete(S[k], removed, axis=0))
    return S


@pytest.fixture(scope="module")
def scenes():
    """the small scan scene, its sphere moved, its second mug removed: cameras,
    colours, and per scene every voxel of the truth (num_points beyond them)"""
    S0 = T.small_scene().arrays()
    pos, R = T.small_cameras()
    f = T.focal(H)
    E = np.tile(np.eye(4), (len(pos), 1, 1))
    E[:, :3, :3], E[:, :3, 3] = R, pos
    colors = np.random.default_rng(1).uniform(0, 1, (16, 3)).astype(np.float32)     # seg ids 10 .. 15
    S = [S0, variant(S0, moved=1), variant(S0, removed=4)]
    assert len(S[2]["draw_id"]) == len(S0["draw_id"]) - 1 and not np.array_equal(S[1]["draw_pos"], S0["draw_pos"])
    every = [C.cloud(s, pos, R, W, H, f, f, W / 2, H / 2, E, 73.0, f, W / 2, H / 2, 5, None, colors, VS, 1 << 30) for s in S]
    assert len({e[0].tobytes() for e in every}) == 3                               # three different clouds
    return dict(S=S, pos=pos, R=R, E=E, f=f, colors=colors, every=every)


def truth_job(scenes, s, num_points):
    """(points, colors, kept, voxels, evals) of scene s at num_points from its voxels"""
    V, F, info = scenes["every"][s]
    if info["voxels"] < num_points:
        return V, F, info["kept"], info["voxels"], 0
    idx, evals, _ = C.bucket_fps(V.astype(np.float64), num_points, 8.0 * VS)
    return V[idx], F[idx], info["kept"], info["voxels"], evals


def batch_args(scenes):
    f = scenes["f"]
    return (scenes["pos"], scenes["R"], W, H, f, f, W / 2, H / 2, scenes["E"], 73.0, f, W / 2, H / 2)


def test_cloud_batch_small_scenes(scenes):
    from mgs.core.engine import scan_cloud, scan_cloud_batch
    nvox = [e[2]["voxels"] for e in scenes["every"]]
    assert min(nvox) > 64
    # two jobs pick (one of them exactly as many as it has voxels), one has fewer voxels than asked, one asks for none
    which, nums = [0, 1, 2, 0], [64, nvox[1], nvox[2] + 1, 0]
    assert nvox[0] >= nums[0] and nvox[1] >= nums[1] and nvox[2] < nums[2]
    res = scan_cloud_batch([scenes["S"][s] for s in which], [scenes["colors"]] * 4, nums, *batch_args(scenes), voxel_size=VS)
    assert len(res) == 4
    for j, (s, m) in enumerate(zip(which, nums)):
        gp, gc, info = res[j]
        tp, tc, kept, voxels, evals = truth_job(scenes, s, m)
        assert gp.dtype == np.float32 and gc.dtype == np.float32 and gp.shape == tp.shape == gc.shape, j
        assert np.array_equal(bits32(gp), bits32(tp)) and np.array_equal(bits32(gc), bits32(tc)), j
        assert len(gp) == min(m, voxels)
        assert (info["kept"], info["voxels"], info["pick_evals"], info["rows"], info["pixels"]) == \
            (kept, voxels, evals, len(tp), 4 * W * H), j
        assert (evals > 0) == (j < 2)
        sp, sc, sinfo = scan_cloud(scenes["S"][s], *batch_args(scenes), scenes["colors"], m, voxel_size=VS)
        assert np.array_equal(bits32(gp), bits32(sp)) and np.array_equal(bits32(gc), bits32(sc)), j
        for key in ("kept", "voxels", "pick_evals", "grid_cells", "rows", "pixels"):
            assert info[key] == sinfo[key], (j, key)
        assert info["render_ms"] > 0 and info["points_compact_ms"] > 0 and info["voxels_ms"] > 0
        assert info["pick_ms"] == res[0][2]["pick_ms"] > 0
    assert scan_cloud_batch([], [], 64, *batch_args(scenes), voxel_size=VS) == []
    # a batch without a pick
    res = scan_cloud_batch([scenes["S"][2]], [scenes["colors"]], nvox[2] + 1, *batch_args(scenes), voxel_size=VS)
    assert len(res[0][0]) == nvox[2] and res[0][2]["pick_ms"] == 0.0 and res[0][2]["pick_evals"] == 0


# -- errors -------------------------------------------------------------------
def raw_jobs(scenes, which, nums, ncolors, rows=80, null_scene=None):
    from mgs.core import abi
    from mgs.scan.scene import pack_scene
    jobs = (abi.ScanCloudJob * len(which))()
    alive = []
    for j, (s, m, nc) in enumerate(zip(which, nums, ncolors)):
        sc, keep = pack_scene(scenes["S"][s])
        oP, oC = np.full((rows, 3), 7.0, np.float32), np.full((rows, 3), 7.0, np.float32)
        alive.append((sc, keep, oP, oC))
        if j != null_scene:
            jobs[j].scene = ctypes.pointer(sc)
        jobs[j].colors = scenes["colors"].ctypes.data_as(PF)
        jobs[j].ncolor, jobs[j].num_points, jobs[j].out_n = nc, m, -5
        jobs[j].out_points, jobs[j].out_colors = oP.ctypes.data_as(PF), oC.ctypes.data_as(PF)
        for i in range(8):
            jobs[j].out_stats[i] = -5
        for i in range(3):
            jobs[j].stage_ms[i] = -5.0
    return jobs, alive


def call_cloud_batch(L, scenes, jobs, voxel_size=VS):
    pos, R, E = (np.ascontiguousarray(scenes[k]) for k in ("pos", "R", "E"))
    f = scenes["f"]
    pick = ctypes.c_double(-5.0)
    rc = L.mgs_scan_cloud_batch(0, len(jobs), jobs, len(pos), pos.ctypes.data_as(PD), R.ctypes.data_as(PD), W, H, f, f,
                                W / 2, H / 2, E.ctypes.data_as(PD), 73.0, f, W / 2, H / 2, 5, None, voxel_size,
                                ctypes.byref(pick))
    return rc, pick.value


def untouched(jobs, alive):
    return all(np.all(oP == 7.0) and np.all(oC == 7.0) for _, _, oP, oC in alive) and \
        all(j.out_n == -5 and list(j.out_stats) == [-5] * 8 and list(j.stage_ms) == [-5.0] * 3 for j in jobs)


def test_cloud_batch_bad_arguments(scenes):
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    EINVAL = abi.MGS["MGS_EINVAL"]
    cases = [(dict(null_scene=1), b"job 1"),                                       # a null scene in job 1 of 3
             (dict(ncolors=[16, 16, 15]), b"job 2"),                               # draw_id 15 has no row of colours
             (dict(nums=[-1, 64, 64]), b"job 0"),
             (dict(voxel_size=0.0), b"voxel_size")]
    for kw, text in cases:
        jobs, alive = raw_jobs(scenes, [0, 1, 2], kw.get("nums", [64, 64, 64]), kw.get("ncolors", [16, 16, 16]),
                               null_scene=kw.get("null_scene"))
        rc, pick = call_cloud_batch(L, scenes, jobs, kw.get("voxel_size", VS))
        err = L.mgs_last_error()
        assert rc == EINVAL, kw
        assert b"mgs_scan_cloud_batch" in err and text in err, err
        assert untouched(jobs, alive) and pick == -5.0, kw
    # ... and the same jobs unharmed work
    jobs, alive = raw_jobs(scenes, [0, 1, 2], [64, 64, 64], [16, 16, 16])
    rc, pick = call_cloud_batch(L, scenes, jobs)
    assert rc == 0 and pick > 0 and [j.out_n for j in jobs] == [64, 64, 64]
    for _, _, oP, oC in alive:
        assert not np.any(oP[:64] == 7.0) and np.all(oP[64:] == 7.0) and np.all(oC[64:] == 7.0)      # beyond out_n: untouched


def test_pick_batch_bad_arguments():
    from mgs.core import abi
    from mgs.core.engine import load_library
    L = load_library()
    EINVAL = abi.MGS["MGS_EINVAL"]
    x = np.random.default_rng(0).uniform(0, 1, (40, 3))
    out = np.full(40, 7, np.int32)
    nev = np.full(4, -5, np.int64)

    def call(pts, off, k, bucket):
        off, k = np.asarray(off, np.int64), np.asarray(k, np.int32)
        return L.mgs_scan_fps_batch(0, len(k), pts.ctypes.data_as(PD), off.ctypes.data_as(PI64), k.ctypes.data_as(PI),
                                    bucket, out.ctypes.data_as(PI), nev.ctypes.data_as(PI64), None)
    off, k = [0, 10, 20, 30, 40], [5, 5, 5, 5]
    bad = x.copy()
    bad[24, 1] = np.inf                                                            # a point of cloud 2
    for args, text in (((bad, off, k, 0.1), b"cloud 2"), ((x, [0, 10, 30, 20, 40], k, 0.1), b"cloud 2"),
                       ((x, off, [5, 11, 5, 5], 0.1), b"cloud 1"), ((x, off, [5, 5, 5, -1], 0.1), b"cloud 3"),
                       ((x, [1, 10, 20, 30, 40], k, 0.1), b"off[0]"), ((x, off, k, 0.0), b"bucket_size"),
                       ((x, off, k, -0.1), b"bucket_size"), ((x, off, k, np.nan), b"bucket_size")):
        assert call(*args) == EINVAL, args[1:]
        err = L.mgs_last_error()
        assert b"mgs_scan_fps_batch" in err and text in err, err
        assert np.all(out == 7) and np.all(nev == -5)
    assert call(x, off, k, 0.1) == 0 and np.all(out[20:] == 7) and np.all(nev > 0)           # beyond the picks: untouched
    for c in range(4):
        assert np.array_equal(out[5 * c:5 * c + 5], C.bucket_fps(x[10 * c:10 * c + 10], 5, 0.1)[0])


# -- the env and the CLI ------------------------------------------------------
@pytest.fixture(scope="module")
def envs():
    """the golden clutter pile as it is, with one object removed, with two"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_clutter_scene import make_env
    from mgs.env.clutter_table import ClutterTableEnv
    z = np.load(os.path.join(HERE, "golden", "clutter_scene.npz"))
    out = []
    for nremoved in range(3):
        base = make_env()
        env = ClutterTableEnv.from_dict({"gripper": base.gripper, "objects": base.objects,
                                         "env_state": {"state": z["state"]}})
        for obj in env.objects[:nremoved]:
            env.remove_obj(obj)
        out.append(env)
    return out


def test_env_scan_clouds_equals_scan_cloud(envs):
    from mgs.env.clutter_table import scan_clouds
    n, w, h, num = 3, 64, 64, 256
    want, infos = [], []
    for e in envs:
        want.append(e.scan_cloud(n, num_points=num, width=w, height=h))
        infos.append(e.last_cloud)
        e.last_cloud = None
    assert len({p.tobytes() for p, _ in want}) >= 2                                   # not one pile three times
    got = scan_clouds(envs, n, num_points=num, width=w, height=h, batch=2)           # a chunk boundary inside
    assert len(got) == 3
    for e, (gp, gc), (wp, wc), info in zip(envs, got, want, infos):
        assert gp.dtype == np.float32 and gp.shape == wp.shape and gc.shape == wc.shape
        assert np.array_equal(bits32(gp), bits32(wp)) and np.array_equal(bits32(gc), bits32(wc))
        for key in ("kept", "voxels", "pick_evals", "grid_cells", "rows", "pixels"):
            assert e.last_cloud[key] == info[key], key
        assert e.last_cloud["render_ms"] > 0


def test_render_scene_processed_cli_ids_key(envs, tmp_path, monkeypatch):
    from mgs.cli import render_scene_processed
    from mgs.env.selector import save_scene
    for k, e in enumerate(envs):
        d = tmp_path / "in" / "Robotiq2f85Gripper" / f"scene_{k:03d}"
        d.mkdir(parents=True)
        save_scene(d / "scene.npz", e.to_dict())
    monkeypatch.setenv("MGS_INPUT_DIR", str(tmp_path / "in"))
    args = ["gripper=robotiq_2f_85", "num_images=3", "width=64", "height=64", "num_points=256", "cloud=device"]
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "many"))
    render_scene_processed.run(args + ["ids=0:3", "batch=2"])
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "all"))
    render_scene_processed.run(args + ["ids=all"])
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "one"))
    sizes = set()
    for k in range(3):
        render_scene_processed.run(args + [f"id={k}"])
        want = np.load(tmp_path / "one" / "Robotiq2f85Gripper" / f"scene_{k:03d}" / "scene_pcd.npz")
        for name in ("many", "all"):
            got = np.load(tmp_path / name / "Robotiq2f85Gripper" / f"scene_{k:03d}" / "scene_pcd.npz")
            assert sorted(got.files) == ["colors", "points"]
            for key in ("points", "colors"):
                assert got[key].dtype == np.float32 and got[key].shape == want[key].shape
                assert np.array_equal(bits32(got[key]), bits32(want[key])), (name, k, key)
        sizes.add(want["points"].tobytes())
    assert len(sizes) >= 2                                                             # not one scene three times
    assert sorted(os.listdir(tmp_path / "many" / "Robotiq2f85Gripper")) == ["scene_000", "scene_001", "scene_002"]
