"""Many scene clouds per call, host side (no GPU): the header's batch entries and
the job struct's mirror, the wrappers' argument checks, the CLI's `ids` key and
its rank slices, and the order in which the batched pick takes its jobs."""
import ctypes
import os
import re

import numpy as np
import pytest


def header_text():
    from mgs.core import abi
    return re.sub(r"/\*.*?\*/", "", open(abi.HEADER).read(), flags=re.S)


def test_header_declares_the_batch_entries():
    from mgs.core import abi
    txt = header_text()
    for f in ("mgs_scan_fps_batch", "mgs_scan_cloud_job_size", "mgs_scan_cloud_batch", "mgs_scan_fps_order"):
        assert re.search(r"^int %s\(" % f, txt, re.M), f
    assert abi.MGS["MGS_ABI_VERSION"] == 24                        # additive entries: the version stays


def test_job_mirror_matches_the_header():
    """this module's own reading of the struct: field names in order, and the
    size their C types give under natural alignment"""
    from mgs.core import abi
    m = re.search(r"typedef struct mgs_scan_cloud_job \{(.*?)\} mgs_scan_cloud_job;", header_text(), re.S)
    assert m, "the header has no mgs_scan_cloud_job"
    names, size, align = [], 0, 1
    widths = {"int32_t": 4, "int64_t": 8, "double": 8, "float": 4}
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        mt = re.match(r"(?:const\s+)?(\w+)\s+(.*)$", decl, re.S)
        ctype, rest = mt.groups()
        for item in rest.split(","):
            mm = re.match(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
            star, name, dim = mm.groups()
            w = ctypes.sizeof(ctypes.c_void_p) if star else widths[ctype]
            size = (size + w - 1) // w * w + w * int(dim or 1)
            align = max(align, w)
            names.append(name)
    size = (size + align - 1) // align * align
    assert [f for f, _ in abi.ScanCloudJob._fields_] == names
    assert ctypes.sizeof(abi.ScanCloudJob) == size
    for f in ("scene", "colors", "ncolor", "num_points", "out_points", "out_colors", "out_n", "out_stats", "stage_ms"):
        assert f in names, f
    assert abi.ScanCloudJob.out_stats.size == 64 and abi.ScanCloudJob.stage_ms.size == 24
    assert isinstance(abi.ScanCloudJob().scene, ctypes.POINTER(abi.ScanScene))


def test_job_mirror_matches_the_library():
    from mgs.core import abi
    from mgs.core.engine import load_library
    assert load_library().mgs_scan_cloud_job_size() == ctypes.sizeof(abi.ScanCloudJob)


def test_batch_wrappers_reject_bad_arguments():
    """shape, dtype and count errors are ValueErrors raised before the library is loaded"""
    from mgs.core import engine
    P = np.zeros((5, 3))
    for clouds, ks in [([P, np.zeros((5, 2))], [1, 1]), ([P, np.zeros(15)], [1, 1]), ([P, P.astype(np.int64)], [1, 1]),
                       ([P, [[0.0, 0.0, 0.0]]], [1, 1]), ([P, P], [1]), ([P], [1, 1]), ([P, P], [1, 6]), ([P, P], [-1, 1]),
                       ([P, P], [1.0, 2.0]), ([P, P], [[1, 1]])]:
        with pytest.raises(ValueError):
            engine.scan_fps_batch(clouds, ks, 0.01)
    for bucket in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            engine.scan_fps_batch([P], [2], bucket)
    good = dict(scenes=[{}, {}], colors=[np.zeros((3, 3))] * 2, num_points=8, cam_pos=np.zeros((2, 3)),
                cam_rot=np.tile(np.eye(3), (2, 1, 1)), width=4, height=4, fx=5.0, fy=5.0, cx=2.0, cy=2.0,
                extrinsics=np.tile(np.eye(4), (2, 1, 1)), pfx=5.0, pfy=5.0, pcx=2.0, pcy=2.0)
    for bad in (dict(colors=[np.zeros((3, 3))]), dict(num_points=[8]), dict(num_points=[8, -1]), dict(num_points=-1),
                dict(colors=[np.zeros((3, 3)), np.zeros((3, 4))]), dict(extrinsics=np.eye(4)[None]),
                dict(cam_rot=np.eye(3)[None]), dict(voxel_size=0.0), dict(region=np.zeros(5)), dict(width=-4)):
        with pytest.raises(ValueError):
            engine.scan_cloud_batch(**dict(good, **bad))


def test_scan_clouds_rejects_envs_on_different_devices():
    from mgs.env.clutter_table import scan_clouds

    class Env:
        def __init__(self, device):
            self.device = device
    with pytest.raises(ValueError, match="different devices"):
        scan_clouds([Env(0), Env(1)], 3)
    with pytest.raises(ValueError, match="batch"):
        scan_clouds([Env(0)], 3, batch=0)
    assert scan_clouds([], 3) == []


# -- the CLI's keys -----------------------------------------------------------
def test_cli_ids_key():
    from mgs.cli import render_scene_processed as R
    from mgs.cli._hydra import compose
    assert R.parse_ids("2:5") == [2, 3, 4]
    assert R.parse_ids("0:3", 3) == [0, 1, 2] and R.parse_ids("4:4") == []
    assert R.parse_ids("all", 4) == [0, 1, 2, 3] and R.parse_ids("all", 0) == []
    for bad, n in (("5:2", None), ("-1:2", None), ("2", None), ("1:2:3", None), ("a:b", None), ("", None), ("0:4", 3),
                   ("all", None)):
        with pytest.raises(ValueError):
            R.parse_ids(bad, n)
    # ids never reaches the YAML reader, which takes 2:5 for a base-60 number
    assert R.split_args(["gripper=panda", "ids=2:5", "cloud=device"]) == ("2:5", False, ["gripper=panda", "cloud=device"])
    assert R.split_args(["id=3", "ids=all"]) == ("all", True, ["id=3"])
    assert R.split_args(["width=64"]) == (None, False, ["width=64"])
    cfg = compose("render_scene_proc", [])
    assert cfg.get("ids") is None and cfg.batch == 64 and cfg.id == 0 and cfg.cloud == "host"      # today's behaviour


@pytest.mark.parametrize("args,match", [(["ids=0:3"], "cloud=device"), (["ids=0:3", "cloud=host"], "cloud=device"),
                                        (["ids=0:3", "cloud=device", "id=1"], "id="), (["ids=5:2", "cloud=device"], "5:2"),
                                        (["ids=all", "cloud=device", "id=0"], "id="),
                                        (["ids=0:3", "cloud=device", "batch=0"], "batch")])
def test_cli_refuses_bad_ids_before_anything_is_read(monkeypatch, tmp_path, args, match):
    from mgs.cli import render_scene_processed as R
    monkeypatch.setenv("MGS_INPUT_DIR", str(tmp_path / "missing"))
    monkeypatch.setenv("MGS_OUTPUT_DIR", str(tmp_path / "out"))
    with pytest.raises(ValueError, match=match):
        R.run(["gripper=robotiq_2f_85"] + args)
    assert not (tmp_path / "out").exists()


def test_cli_rank_slices_are_shard_bounds():
    from mgs.cli import render_scene_processed as R
    from mgs.env.sharding import shard_bounds
    for n, world in ((10, 4), (3, 8), (0, 2), (7, 1), (64, 8)):
        ids = R.parse_ids(f"5:{5 + n}")
        parts = [R.rank_ids(ids, world, r) for r in range(world)]
        for r in range(world):
            lo, hi = shard_bounds(n, world, r)
            assert parts[r] == ids[lo:hi]
        assert sum(parts, []) == ids


# -- the job order ------------------------------------------------------------
def want_order(n, k):
    return sorted(range(len(n)), key=lambda c: (-int(n[c]) * int(k[c]), c))


def test_job_order_rule():
    from mgs.core.engine import scan_fps_order
    rng = np.random.default_rng(5)
    n = rng.integers(0, 50, 200)
    k = np.minimum(rng.integers(0, 50, 200), n)
    got = scan_fps_order(n, k)
    assert got.dtype == np.int32 and sorted(got.tolist()) == list(range(200))          # a permutation
    assert got.tolist() == want_order(n, k)
    work = (n * k)[got]
    assert np.all(work[:-1] >= work[1:])
    # equal work keeps the callers' order, whatever the factors
    assert scan_fps_order([6, 3, 2, 6, 1], [1, 2, 3, 1, 6]).tolist() == [0, 1, 2, 3, 4]
    assert scan_fps_order([4, 9, 4, 9], [2, 3, 2, 3]).tolist() == [1, 3, 0, 2]
    assert scan_fps_order([0, 5, 0], [0, 0, 0]).tolist() == [0, 1, 2]
    assert scan_fps_order([], []).tolist() == []
    # the product is taken in 64 bits
    big = 2 ** 31 - 1
    assert scan_fps_order([big, big, 5], [big - 1, big, 5]).tolist() == [1, 0, 2]
    with pytest.raises(ValueError):
        scan_fps_order([1, 2], [1])
