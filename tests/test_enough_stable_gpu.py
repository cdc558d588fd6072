"""mgs_schedule.enough_stable (ABI 24) on the device: a work-queue launch does
not simulate the candidates it takes after K earlier ones have finished stable.

The contract, checked in every case: the first-K rule over the labels of a
skipping run equals the rule over the oracle's full run, and every entry that
was not skipped is the oracle's bit for bit.  On a grid of g = 2 workgroups
without rotation the candidates that ran form a prefix [0, s) of the launch
holding at most K + g - 1 stable ones (when the last unskipped index was taken,
at most K - 1 had finished stable and at most g were in flight), which bounds
the cut from both sides.

256 seeded Robotiq x cracker-box candidates at h200; the oracle at 64 contacts
/ 256 rows gives 41 collision-free ones (7, 9, 16, 19, 20, 23, ...), labels
1, 1, 1, 1, 0, 1, ... (29 stable), none over 14 contacts / 57 rows, so the main
capacity never escalates."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
except Exception:  # pragma: no cover - CPU containers
    pass

from mgs.core.abi import MGS  # noqa: E402

SKIPPED, FAIL_SKIPPED = MGS.get("MGS_FLAG_SKIPPED"), MGS.get("MGS_FAIL_SKIPPED")
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("label", "fail_step", "obj_qpos", "stats")


@contextlib.contextmanager
def queue_mode(mode, *engines):
    """mgs_rollout_queue(mode) on the libraries of these engines, restored on exit"""
    libs = {id(e.lib): e.lib for e in engines}.values()
    prev = [(L, L.mgs_rollout_queue(-1)) for L in libs]
    try:
        for L in libs:
            L.mgs_rollout_queue(mode)
        yield
    finally:
        for L, p in prev:
            L.mgs_rollout_queue(p)


@pytest.fixture(scope="module")
def ref(env, candidates):
    """the oracle's full run, computed once: mask over the 256, the plan of the
    collision-free ones and their rollout at 64 contacts / 256 rows"""
    from conftest import plan_for
    from oracle import oracle as O
    poses, J = candidates
    q, mp, mq, _ = env.initial_state(poses, J)
    om = O.OracleModel(env.model, ncon_max=64, nefc_max=256)
    free = om.collision_free(q, mp, mq, nthreads=8)
    idx = np.nonzero(free)[0]
    plan = plan_for(env, poses[idx], J[idx])
    ro = om.rollout(plan, nthreads=8)
    assert len(idx) == 41 and idx[:6].tolist() == [7, 9, 16, 19, 20, 23]
    assert ro["label"][:6].astype(int).tolist() == [1, 1, 1, 1, 0, 1] and int(ro["label"].sum()) == 29
    assert ro["stats"][:, 0].max() <= 14 and ro["stats"][:, 1].max() <= 57 and not ro["stats"][:, 2].any()
    return dict(q=q, mp=mp, mq=mq, free=free, idx=idx, plan=plan, ro=ro, full_plan=plan_for(env, poses, J))


def _check(res, ro, plan, K, lo=None, hi=None):
    """the contract on a result over the oracle's candidates; returns s, the
    start of the skipped suffix (lo <= s <= hi where given)"""
    from mgs.env.gravityless_object_grasping import apply_enough_stable
    n = len(ro["label"])
    assert np.array_equal(apply_enough_stable(res["label"], K), apply_enough_stable(ro["label"], K))
    sk = (res["stats"][:, 2] & SKIPPED) != 0
    s = int(np.nonzero(sk)[0][0]) if sk.any() else n
    assert sk[s:].all() and not sk[:s].any(), f"the skipped set is no suffix: {np.nonzero(sk)[0].tolist()}"
    before = np.cumsum(ro["label"]) - ro["label"]
    assert np.all(before[sk] >= K)
    a = plan.obj_qposadr
    assert np.all(res["fail_step"][sk] == FAIL_SKIPPED) and not res["label"][sk].any()
    assert np.array_equal(res["obj_qpos"][sk], plan.qpos_init[sk, a:a + 7])
    assert np.all(res["stats"][sk] == np.array([0, 0, SKIPPED, 0, 0, 0]))
    for k in KEYS:
        assert np.array_equal(res[k][~sk], ro[k][~sk]), k
    print(f"enough_stable={K}: skipped suffix starts at s={s} of {n}")
    if lo is not None:
        assert lo <= s, (s, lo)
    if hi is not None:
        assert s <= hi, (s, hi)
    return s


def _sliced(env, plan, K, yield_every, engine=None, engine_for=None, cap=None, max_ncon=None):
    from mgs.env.gravityless_object_grasping import sliced_rollout
    return sliced_rollout(plan, engine or env.engine, engine_for or env.engine_for, cap or env.ncon_max,
                          max_ncon or env.MAX_NCON, 1, yield_every=yield_every, enough_stable=K)


def test_stability_call_skips_behind_k(env, ref):
    with queue_mode(2, env.engine):
        res = _sliced(env, ref["plan"], 3, 0)
    s = _check(res, ref["ro"], ref["plan"], 3, lo=3, hi=5)
    assert res["skipped"] == 41 - s and res["overflow"] == 0


def _fused(eng, sched, ref, dev):
    """one mgs_mask_rollout_device launch over the 256; host copies of its outputs"""
    from mgs.core import abi
    n = len(ref["q"])
    fp = ref["full_plan"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    dq, dmp, dmq, dps, dpt = t(ref["q"]), t(ref["mp"]), t(ref["mq"]), t(fp.phase_start), t(fp.phase_target)
    o = dict(free=torch.zeros(n, dtype=torch.uint8, device=dev), label=torch.zeros(n, dtype=torch.uint8, device=dev),
             fail_step=torch.zeros(n, dtype=torch.int32, device=dev),
             obj_qpos=torch.zeros((n, 7), dtype=torch.float64, device=dev),
             stats=torch.zeros((n, abi.MGS["MGS_NSTATS"]), dtype=torch.int32, device=dev),
             rec=torch.zeros((n, eng.resume_width()), dtype=torch.float64, device=dev))
    eng.mask_rollout_device(sched, n, dq.data_ptr(), dmp.data_ptr(), dmq.data_ptr(), dps.data_ptr(), dpt.data_ptr(),
                            o["free"].data_ptr(), o["label"].data_ptr(), o["fail_step"].data_ptr(),
                            o["obj_qpos"].data_ptr(), o["stats"].data_ptr(), d_resume_out=o["rec"].data_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["label"] = out["label"].astype(bool)
    return out


def test_fused_launch_masks_everything_and_zeroes_its_count(env, ref):
    from mgs.core import abi
    eng, fp, idx, free = env.engine, ref["full_plan"], ref["idx"], ref["free"]
    dev = torch.device("cuda", 0)

    def sched(K):
        s = abi.make_schedule(fp.nsteps, fp.check_every, fp.check_at_end, fp.ctrl, fp.obj_qposadr,
                              check_offset=getattr(fp, "check_offset", None))
        s.enough_stable = K
        return s

    def check(o, K):
        # masks are computed behind the cut too; rejects keep the reject outputs
        assert np.array_equal(o["free"].astype(bool), free)
        rej = np.nonzero(~free)[0]
        assert np.all(o["fail_step"][rej] == -2) and not o["stats"][rej].any() and not o["label"][rej].any()
        sub = {k: o[k][idx] for k in KEYS}
        if K == 0:
            for k in KEYS:
                assert np.array_equal(sub[k], ref["ro"][k]), k
            return None
        s = _check(sub, ref["ro"], ref["plan"], K, lo=3, hi=5)
        # the skipped collision-free candidates are those with index >= c, for one 17 <= c <= 23
        lu, fs = int(idx[s - 1]), int(idx[s])
        assert lu + 1 <= 23 and fs >= 17, (lu, fs)
        return s

    with queue_mode(2, eng):
        check(_fused(eng, sched(3), ref, dev), 3)
        check(_fused(eng, sched(0), ref, dev), 0)
        # the queue headers cycle through 64 slots: after 64 more launches every
        # slot, the first launch's included, has been used again after a
        # counting launch; a count that was not returned to zero would skip
        # from the first index on (s < 3)
        for _ in range(64):
            check(_fused(eng, sched(3), ref, dev), 3)


def test_rotation_on(env, ref):
    """yielded candidates are not in flight on a workgroup, so there is no upper
    bound on s; no candidate is lost and no ring spin expires"""
    with queue_mode(2, env.engine):
        res = _sliced(env, ref["plan"], 3, 7)
        spins = env.engine.queue_stats()[1]
    _check(res, ref["ro"], ref["plan"], 3, lo=3)
    assert not (res["fail_step"] == MGS["MGS_FAIL_YIELDED"]).any()
    assert spins == 0


def test_off_switches(env, ref):
    with queue_mode(0, env.engine):
        res = _sliced(env, ref["plan"], 3, 0)
    assert res["skipped"] == 0
    for k in KEYS:
        assert np.array_equal(res[k], ref["ro"][k]), k
    assert type(env).WORK_SKIP is True
    try:
        env.WORK_SKIP = False
        with queue_mode(2, env.engine):
            off = env.rollout(ref["plan"], enough_stable=3)
    finally:
        del env.WORK_SKIP
    assert off["skipped"] == 0
    for k in KEYS:
        assert np.array_equal(off[k], ref["ro"][k]), k


def test_escalation_skips_in_the_escalation_launch(env, ref):
    """main capacity 4 contacts, doubled to 8 and 16: most of the 41 overflow the
    main launch, so their labels, and the skip, come from the escalation"""
    from mgs.core.engine import Engine
    engines = {c: Engine(env.model, device=env.device, ncon_max=c) for c in (4, 8, 16, 32)}
    try:
        with queue_mode(2, *engines.values()):
            first = engines[4].rollout(ref["plan"], resumable=True)
            res = _sliced(env, ref["plan"], 3, 0, engine=engines[4], engine_for=engines.__getitem__, cap=4,
                          max_ncon=32)
    finally:
        for e in engines.values():
            e.close()
    assert ((first["stats"][:, 2] & MGS["MGS_FLAG_CAPACITY"]) != 0).sum() > 20
    from mgs.env.gravityless_object_grasping import apply_enough_stable
    ro = ref["ro"]
    assert np.array_equal(apply_enough_stable(res["label"], 3), apply_enough_stable(ro["label"], 3))
    sk = (res["stats"][:, 2] & SKIPPED) != 0
    assert res["skipped"] == int(sk.sum()) > 0 and res["overflow"] == 0
    before = np.cumsum(ro["label"]) - ro["label"]
    assert np.all(before[sk] >= 3)
    for k in ("label", "fail_step", "obj_qpos"):
        assert np.array_equal(res[k][~sk], ro[k][~sk]), k


@pytest.fixture(scope="module")
def senv():
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_clutter_scene import make_env
    e = make_env("ShadowHand")
    e.set_state(np.load(os.path.join(HERE, "golden", "clutter_scene_shadow.npz"))["state"])
    return e


@pytest.fixture(scope="module")
def scand(senv):
    from mgs.sampler.antipodal import hand_candidates
    from mgs.util.geo.transforms import SE3Pose
    Hs, Js = [], []
    for k, o in enumerate(senv.objects):
        h, j, _ = hand_candidates(o, 32, senv.gripper, seed=k)
        Hs.append((senv.get_obj_pose(o.name) @ SE3Pose.from_mat(h)).to_mat())
        Js.append(j)
    return SE3Pose.from_mat(np.concatenate(Hs).astype(np.float32)), np.concatenate(Js)


def test_shadow_pile_skips_in_the_escalation(senv, scand):
    """wide build: the 11 collision-free pile candidates have 19 to 24 contacts
    at their maximum (oracle at 128 / 256: labels 0 0 0 1 1 1 0 0 1 0 1); where
    that is over the env's main capacity they all escalate, and the skip
    happens in the escalation launch"""
    from conftest import full_capacity_oracle
    from mgs.env.gravityless_object_grasping import apply_enough_stable
    poses, J = scand
    st = senv.get_state()
    idx = np.nonzero(senv.grasp_collision_mask(poses, J))[0]
    assert len(idx) == 11
    plan = senv.stable_plan(poses[idx], J[idx], st, nstep_lift=200, close_steps=200)
    ro = full_capacity_oracle(senv, st).rollout(plan, nthreads=8)
    assert ro["label"].astype(int).tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1]
    with queue_mode(2, senv.engine_for_state(st)):
        res = senv.grasp_stable_mask(poses[idx], J[idx], st, nstep_lift=200, close_steps=200, enough_stable=1,
                                     return_details=True)
    assert np.array_equal(res["label"], apply_enough_stable(ro["label"], 1))
    sk = (res["stats"][:, 2] & SKIPPED) != 0
    s = int(np.nonzero(sk)[0][0]) if sk.any() else 11
    print(f"shadow pile: skipped suffix starts at s={s}, skipped {res['skipped']}")
    assert sk[s:].all() and not sk[:s].any()
    assert 4 <= s <= 5
    assert res["skipped"] == 11 - s
    for k in ("fail_step", "obj_qpos"):
        assert np.array_equal(res[k][~sk], ro[k][~sk]), k
