"""Host side of the enough_stable work skip (ABI 24): the header's new field,
flag and fail code through mgs.core.abi, and sliced_rollout's pruning against a
fake engine with tests/test_sliced_rollout.py's contract plus the skip.

The fake skips candidate k of a launch when at least `enough_stable` earlier
candidates of that launch ended with label 1: the kernel's most eager case (a
grid of one workgroup).  The contract checked: the first-K rule over the
labels of a skipping run equals the rule over a full run's, and nothing is
skipped that the rule would keep.  CPU only; the kernel's side is
tests/test_enough_stable_gpu.py."""
import numpy as np
import pytest

from mgs.core import abi
from mgs.core.abi import MGS
from mgs.env.gravityless_object_grasping import (CapacityError, RolloutPlan, apply_enough_stable,
                                                 sliced_rollout)

CAP, PAUSED, NS = MGS["MGS_FLAG_CAPACITY"], MGS["MGS_FLAG_PAUSED"], MGS["MGS_NSTATS"]
H = 60


def test_abi_has_the_field_the_flag_and_the_fail_code():
    assert MGS["MGS_ABI_VERSION"] == 24
    assert MGS["MGS_FLAG_SKIPPED"] == 16
    assert MGS["MGS_FAIL_SKIPPED"] == -6
    names = [f[0] for f in abi.Schedule._fields_]
    assert names[-1] == "enough_stable" and names[-2] == "yield_every"
    s = abi.make_schedule([10, 20], [0, 5], [1, 1], [np.zeros(2), np.zeros(2)], obj_qposadr=3)
    assert s.enough_stable == 0


class SkipFakeEngine:
    """tests/test_sliced_rollout.py's fake (candidate i needs need[i, t]
    contacts at step t and fails at fail_at[i]; a record is [step, sumcon,
    flags]) with mgs_schedule.enough_stable: candidate k of a launch is skipped
    when at least enough_stable earlier ones of the launch ended with label 1"""

    def __init__(self, need, fail_at, cap, log):
        self.need, self.fail_at, self.cap, self.log = need, fail_at, cap, log

    def rollout(self, plan, resumable=False, resume_from=None, pause_step=0, capped_continue=False, yield_every=0,
                enough_stable=0):
        ids = plan.qpos_init[:, 0].astype(int)
        self.log.append(dict(cap=self.cap, ids=ids.copy(), pause=pause_step, resumed=resume_from is not None,
                             K=enough_stable))
        n = len(ids)
        out = dict(label=np.zeros(n, bool), fail_step=np.zeros(n, np.int32), obj_qpos=np.zeros((n, 7)),
                   stats=np.zeros((n, NS), np.int32), resume=np.zeros((n, 4)))
        stable = 0
        for k, i in enumerate(ids):
            if enough_stable > 0 and stable >= enough_stable:
                out["fail_step"][k] = MGS["MGS_FAIL_SKIPPED"]
                out["obj_qpos"][k] = plan.qpos_init[k, plan.obj_qposadr:plan.obj_qposadr + 7]
                out["stats"][k, 2] = MGS["MGS_FLAG_SKIPPED"]
                continue
            t0, sc = (int(resume_from[k, 0]), int(resume_from[k, 1])) if resume_from is not None else (0, 0)
            rf = int(resume_from[k, 2]) if resume_from is not None else 0
            flags, label, fs = (rf & ~PAUSED) if rf & PAUSED else 0, True, -1
            t = t0
            while t < H:
                if pause_step > 0 and t >= pause_step:
                    flags |= PAUSED
                    out["resume"][k] = (t, sc, flags, 0)
                    label, fs = False, -4
                    break
                if self.need[i, t] > self.cap:
                    flags |= CAP
                    if not capped_continue:
                        out["resume"][k] = (t, sc, flags, 0)
                        label, fs = False, -3
                        break
                sc += int(min(self.need[i, t], self.cap))
                if t == self.fail_at[i]:
                    label, fs = False, t
                    break
                t += 1
            stable += bool(label)
            out["label"][k] = label
            out["fail_step"][k] = fs
            out["obj_qpos"][k] = i + np.arange(7)
            out["stats"][k, 2] = flags
            out["stats"][k, 4] = sc
        return out


def _case(seed, n=40):
    rng = np.random.default_rng(seed)
    need = rng.integers(0, 10, (n, H))
    need[rng.random((n, H)) < 0.03] = rng.integers(10, 50)      # rare spikes past the main capacity
    fail_at = np.where(rng.random(n) < 0.4, rng.integers(0, H, n), -1)
    q = np.zeros((n, 8))
    q[:, 0] = np.arange(n)
    q[:, 1:] = rng.standard_normal((n, 7))
    z = np.zeros((n, 5, 3))
    plan = RolloutPlan(nsteps=[H], check_every=[0], check_at_end=[1], ctrl=[np.zeros(1)], qpos_init=q,
                       mocap_quat=np.zeros((n, 4)), phase_start=z, phase_target=z, obj_qposadr=1)
    return need, fail_at, plan


def _run(need, fail_at, plan, slices, K, **kw):
    log, engines = [], {}

    def engine_for(c):
        return engines.setdefault(c, SkipFakeEngine(need, fail_at, c, log))
    res = sliced_rollout(plan, engine_for(10), engine_for, 10, 80, slices, yield_every=32, enough_stable=K, **kw)
    return res, log


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("K", [1, 3, 1000])
def test_first_k_rule_is_unchanged_by_the_skip(seed, slices, K):
    need, fail_at, plan = _case(seed)
    full, _ = _run(need, fail_at, plan, slices, None)
    res, log = _run(need, fail_at, plan, slices, K)
    assert np.array_equal(apply_enough_stable(res["label"], K), apply_enough_stable(full["label"], K))
    skipped = (res["stats"][:, 2] & MGS["MGS_FLAG_SKIPPED"]) != 0
    assert res["skipped"] == int(skipped.sum()) and full["skipped"] == 0
    before = np.cumsum(full["label"]) - full["label"]        # stable labels of the full run before each index
    assert np.all(before[skipped] >= K)
    # a skipped entry as the kernel writes it; any other entry is the full run's
    a = plan.obj_qposadr
    assert not res["label"][skipped].any() and np.all(res["fail_step"][skipped] == MGS["MGS_FAIL_SKIPPED"])
    assert np.array_equal(res["obj_qpos"][skipped], plan.qpos_init[skipped, a:a + 7])
    assert np.all(res["stats"][skipped][:, [0, 1, 3, 4, 5]] == 0)
    for k in ("label", "fail_step", "obj_qpos", "stats"):
        assert np.array_equal(res[k][~skipped], full[k][~skipped]), k
    # no escalation or slice launch holds a candidate the pruning should have
    # dropped, and each carries K minus the final stable labels before its first
    assert log[0]["K"] == K and len(log[0]["ids"]) == len(need)
    _replay_launches(need, fail_at, plan, log, K)
    if K == 1:
        assert res["skipped"] > 0


def _replay_launches(need, fail_at, plan, log, K):
    """run the logged launches again on a fresh fake, tracking the labels the
    host holds after each, and check every launch after the first against the
    pruning rule"""
    n = len(need)
    label = np.zeros(n, bool)
    rec = np.zeros((n, 4))
    for j, c in enumerate(log):
        ids = c["ids"]
        if j > 0:
            known = np.cumsum(label) - label
            assert np.all(np.diff(ids) > 0)
            assert np.all(known[ids] < K), "a launch holds a candidate behind K final stable labels"
            assert c["K"] == K - known[ids[0]] and c["K"] >= 1
        last = c["cap"] >= 80
        sub = SkipFakeEngine(need, fail_at, c["cap"], []).rollout(
            plan.subset(ids), resumable=True, resume_from=rec[ids] if c["resumed"] else None, pause_step=c["pause"],
            enough_stable=c["K"])
        assert not last or not (sub["stats"][:, 2] & CAP).any()
        label[ids] = sub["label"]
        rec[ids] = sub["resume"]


def test_no_capacity_error_behind_k():
    """the only candidate over the last capacity lies behind the first K stable
    ones: the reference never simulates it, so the call does not fail (it does
    without enough_stable)"""
    need, fail_at, plan = _case(3)
    full, _ = _run(need, fail_at, plan, 1, None)
    i = int(np.nonzero(np.cumsum(full["label"]) >= 2)[0][0]) + 3      # behind the second stable one
    need[i, 20] = 500
    fail_at[i] = -1
    with pytest.raises(CapacityError):
        _run(need, fail_at, plan, 1, None)
    res, log = _run(need, fail_at, plan, 1, 2)
    assert res["stats"][i, 2] & MGS["MGS_FLAG_SKIPPED"] and res["fail_step"][i] == MGS["MGS_FAIL_SKIPPED"]
    need2, fail2, _ = _case(3)
    full2, _ = _run(need2, fail2, plan, 1, None)
    assert np.array_equal(apply_enough_stable(res["label"], 2), apply_enough_stable(full2["label"], 2))
    # ... and one in front of them still fails the call
    j = int(np.nonzero(full["label"])[0][0])
    need[j, 20] = 500
    with pytest.raises(CapacityError) as ei:
        _run(need, fail_at, plan, 1, 2)
    assert j in ei.value.candidates.tolist()


def test_off_keeps_the_old_engine_signature():
    """enough_stable=None: engine.rollout is called with exactly the keywords it
    always had (the fake of tests/test_sliced_rollout.py does not take the new
    one)"""
    from test_sliced_rollout import FakeEngine, _case as old_case
    need, fail_at, plan = old_case(1)
    log, engines = [], {}

    def engine_for(c):
        return engines.setdefault(c, FakeEngine(need, fail_at, c, log))
    ref = FakeEngine(need, fail_at, 10 ** 6, []).rollout(plan)
    for kw in ({}, dict(enough_stable=None)):
        res = sliced_rollout(plan, engine_for(10), engine_for, 10, 80, 3, yield_every=32, **kw)
        assert np.array_equal(res["label"], ref["label"]) and res["skipped"] == 0
    with pytest.raises(TypeError):
        sliced_rollout(plan, engine_for(10), engine_for, 10, 80, 3, yield_every=32, enough_stable=2)


def test_env_switches():
    """WORK_SKIP off passes no K; a call that can skip runs without rotation
    unless yield_every is given"""
    from mgs.env.clutter_table import ClutterTableEnv
    from mgs.env.gravityless_object_grasping import GravitylessObjectGrasping

    for cls in (GravitylessObjectGrasping, ClutterTableEnv):
        e = cls.__new__(cls)
        assert cls.WORK_SKIP is True
        assert e.skip_setting(100, 3, None) == (3, cls.SKIP_YIELD_EVERY) and cls.SKIP_YIELD_EVERY == 0
        assert e.skip_setting(100, 3, 7) == (3, 7)
        assert e.skip_setting(100, 1000, None) == (1000, cls.YIELD_EVERY)
        assert e.skip_setting(100, None, None) == (None, cls.YIELD_EVERY)
        e.WORK_SKIP = False
        assert e.skip_setting(100, 3, None) == (None, cls.YIELD_EVERY)


def test_cli_evaluators_pass_k():
    """_common.evaluators hands K to the stability stage: the keyword, else the
    configuration's enough_stable, else nothing"""
    from mgs.cli import _common

    class Env:
        grasp_collision_mask = None

        def grasp_stability_evaluation_from_joints(self, p, j, **kw):
            return kw

    cfg = {"horizon": "h200"}
    assert "enough_stable" not in _common.evaluators(Env(), cfg)[1](None, None)
    assert _common.evaluators(Env(), cfg, enough_stable=7)[1](None, None)["enough_stable"] == 7
    assert _common.evaluators(Env(), dict(cfg, enough_stable=1000))[1](None, None)["enough_stable"] == 1000
    assert _common.evaluators(Env(), dict(cfg, enough_stable=1000), enough_stable=5)[1](None, None)["enough_stable"] == 5
