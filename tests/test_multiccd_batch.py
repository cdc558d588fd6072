"""multiccd's perturbed MPRs of several small pairs in one lockstep call
(mgs_kernels.hip multiccd_x: 16 groups of 4 lanes, group g running
perturbation g & 3 of the pair in slot g >> 2; lane li of a group holds
vertices li and li + 4 of both hulls).

Small synthetic models (nv 14, 20 or 28: the generic library's kernels, no code
object is compiled) with the multiccd flag on, as tests/test_group_support.py:
meshes of at most 8 vertices stand a fraction of a millimetre inside the box
floor or inside each other, in several states each (unrotated, turned at
random by small and large angles, resting on a hull face).  Ten free-simulation
steps on the GPU are compared bit for bit with the oracle's.  The cases put
two, three, four and more than four such pairs into one step, hulls of 4, 5
and 8 vertices (with 5 some lanes of a quad hold one vertex, others two), a
tapered box lying flat whose tied bottom vertices sit in lanes out of index
order, a capsule (rounding radius) on a mesh, a hovering body whose pair
misses among hitting ones, a big-hull pair and a box-box pair between two
small ones (the stored results must survive them) and one small pair alone
(the path of a pair on its own).
CPU: the oracle's contact counts against the capacity used, the number of
eligible pairs hitting in one step, and the tie structure of the flat box."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

NCON = 40           # contact capacity of every case (asserted unused to the full on the oracle)
NSTEPS = 10
DEPTH = 3e-4        # initial penetration
FLOOR_TOP = 0.02

HEAD = """<mujoco><option cone="elliptic" integrator="implicitfast"><flag multiccd="enable"/></option>
<asset>{assets}</asset>
<worldbody>
  <body name="floor"><geom name="floor" type="box" size="0.3 0.2 0.02"/></body>
{bodies}{idle}
</worldbody></mujoco>"""
# one-dof bodies that touch nothing: they bring the dof count to one the library is built for
IDLE = """  <body pos="1 {y} 1"><joint type="hinge" axis="0 1 0"/><geom type="sphere" size="0.01" contype="0" conaffinity="0"/></body>
"""


def sphere_points(n, r=0.02):
    """n points on a sphere (golden-angle spiral): every one is a hull vertex"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return (r * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(np.float32).astype(np.float64)


def taper_points():
    """a box widening upwards, symmetric in x and y (the principal axes are x,
    y, z and the mesh frame is the input's moved to the centre of mass): the
    bottom face is a
    rectangle whose four vertices tie for the direction (0, 0, -1), and pairs
    of them for every direction without an x or without a y component.  The
    wider top face sorts first and last in the compiled (lexicographic) vertex
    order, so the bottom face takes the indices 2, 3, 4, 5"""
    bot = [[sx * 0.008, sy * 0.012, -0.03] for sx in (-1, 1) for sy in (-1, 1)]
    top = [[sx * 0.012, sy * 0.018, 0.03] for sx in (-1, 1) for sy in (-1, 1)]
    return np.array(bot + top, np.float32).astype(np.float64)


def cuboid_points(hx=0.015, hy=0.011, hz=0.008):
    s = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64)
    return (s * [hx, hy, hz]).astype(np.float32).astype(np.float64)


def quat_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def small_quat(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * ax])


def face_down_quat(pts):
    """the rotation that puts the hull's most downward face flat on the floor"""
    from scipy.spatial import ConvexHull
    nrm = ConvexHull(pts).equations[:, :3]
    n = nrm[np.argmin(nrm[:, 2])]
    ax = np.cross(n, [0.0, 0.0, -1.0])
    s = np.linalg.norm(ax)
    if s < 1e-12:       # already flat
        return np.array([1.0, 0, 0, 0])
    ang = np.arctan2(s, -n[2])
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax / s])


def mesh_xml(name, pts):
    return f'<mesh name="{name}" vertex="{" ".join(repr(float(x)) for x in pts.ravel())}"/>'


# a shape: (geom xml, points of its convex cores in the body frame, rounding radius)
def mesh_shape(name, pts):
    return (f'<geom type="mesh" mesh="{name}"/>', pts, 0.0)


def twin_shape(name, pts, dx=0.03):
    """the same mesh twice in one body, side by side: two pairs per body"""
    off = np.array([dx, 0.0, 0.0])
    return (f'<geom type="mesh" mesh="{name}" pos="{-dx} 0 0"/><geom type="mesh" mesh="{name}" pos="{dx} 0 0"/>',
            np.concatenate([pts - off, pts + off]), 0.0)


def capsule_shape(r=0.006, h=0.012):
    # lying along x
    c = np.cos(np.pi / 4)
    return (f'<geom type="capsule" size="{r} {h}" quat="{c} 0 {c} 0"/>', np.array([[-h, 0, 0], [h, 0, 0.0]]), r)


def box_shape(hx=0.015, hy=0.012, hz=0.01):
    s = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64)
    return (f'<geom type="box" size="{hx} {hy} {hz}"/>', s * [hx, hy, hz], 0.0)


class Case:
    """bodies standing in columns on the floor: columns[c] lists the shapes of
    column c from the floor up; every body DEPTH inside the one below it.
    states: one initial qpos per entry of `tilts` (None: unrotated; (seed,
    angle): every body turned by a random rotation of that angle; "face": every
    hull resting on a face, so that multiccd's tilted MPRs find its corners)."""

    def __init__(self, assets, columns, tilts, gap_columns=()):
        self.assets, self.columns, self.tilts, self.gap_columns = assets, columns, tilts, gap_columns
        self.nbody = sum(len(c) for c in columns)
        nidle = {2: 2, 3: 2, 4: 4}[self.nbody]
        bodies = "".join(f'  <body name="b{i}" pos="0 0 {1 + i}"><freejoint/>{sh[0]}</body>\n'
                         for i, sh in enumerate(s for c in columns for s in c))
        self.xml = HEAD.format(assets="".join(assets), bodies=bodies,
                               idle="".join(IDLE.format(y=j) for j in range(nidle)))
        self.nidle = nidle

    def qpos(self, tilt):
        rng = np.random.default_rng(tilt[0]) if isinstance(tilt, tuple) else None
        out = []
        xs = 0.12 * (np.arange(len(self.columns)) - 0.5 * (len(self.columns) - 1))
        for c, col in enumerate(self.columns):
            top = None                                     # the highest point so far of this column
            lift = 5e-4 if c in self.gap_columns else -DEPTH   # a gap column hovers: its pair misses
            for _, pts, rad in col:
                if tilt == "face":
                    q = face_down_quat(pts) if len(pts) >= 4 else np.array([1.0, 0, 0, 0])
                else:
                    q = small_quat(rng, tilt[1]) if tilt else np.array([1.0, 0, 0, 0])
                w = pts @ quat_mat(q).T
                lo = w[np.argmin(w[:, 2])]
                if top is None:     # centred on the column's axis, its lowest point in the floor
                    pos = np.array([xs[c], 0.0, FLOOR_TOP + lift + rad - lo[2]])
                else:               # its lowest point in the highest point of the body below
                    pos = top + [0, 0, lift + rad] - lo
                out.append(np.concatenate([pos, q]))
                hi = w[np.argmax(w[:, 2])]
                top = pos + hi + [0, 0, rad]
                lift = -DEPTH
        return np.concatenate(out + [np.zeros(self.nidle)])

    @functools.cached_property
    def cm(self):
        from mgs.core.mjcf import compile_xml
        cm = compile_xml(self.xml)
        assert cm.nv == 6 * self.nbody + self.nidle and cm.nq == 7 * self.nbody + self.nidle
        return cm

    @functools.cached_property
    def plan(self):
        q = np.stack([self.qpos(t) for t in self.tilts])
        n = len(q)
        mp = np.zeros((n, 1, 3))
        return SimpleNamespace(nsteps=[NSTEPS], check_every=[0], check_at_end=[0], ctrl=[np.zeros(int(self.cm.nu))],
                               obj_qposadr=-1, check_offset=None, qpos_init=q,
                               mocap_quat=np.tile([1.0, 0, 0, 0], (n, 1)), phase_start=mp, phase_target=mp.copy())

    def rows(self):
        from mgs.core.engine import default_rows
        return default_rows(self.cm, int(self.cm.pack(ncon_max=NCON)[0]["nefc_max"]))

    @functools.cached_property
    def oracle(self):
        """the reference, computed once per case and shared"""
        from oracle import oracle as O
        om = O.OracleModel(self.cm, ncon_max=NCON, nefc_max=self.rows())
        r = om.simulate_batch(self.plan, nthreads=4)
        for v in r.values():
            v.setflags(write=False)
        return r

    def eligible_pairs(self):
        """the geom pairs whose multiccd may go several at a time: kind CONVEX,
        both hulls of at most 8 vertices, no cylinder (multiccd_q<8>'s pairs)"""
        from mgs.core import mjcf
        cm = self.cm
        g1, g2, kind = cm.pair_table(cm.ccd_mode())
        assert len(g1) <= 64          # one batch of the narrowphase
        nvert = np.asarray(cm.hull_vertnum)[np.asarray(cm.geom_hullid)]
        cyl = np.asarray(cm.geom_type) == mjcf.GEOM_TYPES["cylinder"]
        return [tuple(sorted((int(a), int(b)))) for a, b, k in zip(g1, g2, kind)
                if k == mjcf.PAIR_CONVEX and nvert[a] <= 8 and nvert[b] <= 8 and not (cyl[a] or cyl[b])]

    def touching(self, tilt):
        """the geom pairs with a contact in the oracle's first step of a state, in contact order"""
        from oracle import oracle as O
        om = O.OracleModel(self.cm, ncon_max=NCON, nefc_max=self.rows())
        n, p, fr, dist, g = om.contacts(self.qpos(tilt), np.zeros(3), np.array([1.0, 0, 0, 0]), maxc=NCON)
        assert n < NCON
        out = []
        for x in g.tolist():
            t = tuple(sorted(x))
            if t not in out:
                out.append(t)
        return out


TILTS = [None, (1, 0.05), (2, 0.3), (3, 1.0), "face"]


@functools.lru_cache(maxsize=None)
def case(name):
    m4, m5, m8, tp, cb = sphere_points(4), sphere_points(5), sphere_points(8), taper_points(), cuboid_points()
    big, m20 = sphere_points(186, 0.03), sphere_points(20)
    assets = [mesh_xml("m4", m4), mesh_xml("m5", m5), mesh_xml("m8", m8), mesh_xml("tp", tp), mesh_xml("cb", cb),
              mesh_xml("big", big), mesh_xml("m20", m20)]
    s4, s5, s8, st, sc = (mesh_shape("m4", m4), mesh_shape("m5", m5), mesh_shape("m8", m8), mesh_shape("tp", tp),
                          mesh_shape("cb", cb))
    if name == "x2":
        return Case(assets, [[s8], [s5]], TILTS)
    if name == "x3":
        return Case(assets, [[s8], [s5], [s4]], TILTS)
    if name == "x4":
        return Case(assets, [[s8], [s5], [s4], [st]], TILTS)
    if name == "x8":
        # more than four in one batch: two meshes per body, eight pairs with the floor
        return Case(assets, [[twin_shape("m8", m8)], [twin_shape("m5", m5)], [twin_shape("m4", m4)],
                             [twin_shape("tp", tp)]], TILTS)
    if name == "stack":
        # two columns of two: hull-hull pairs without the box among the four
        return Case(assets, [[s8, s5], [st, s4]], TILTS)
    if name == "flat":
        # flat and unrotated (state 0: the bottom faces tie), and slightly tilted
        return Case(assets, [[st], [sc]], [None, (4, 1e-3), (5, 0.02)])
    if name == "round":
        # a capsule lying on a mesh: kind CONVEX with a rounding radius
        return Case(assets, [[s8, capsule_shape()], [s5]], TILTS)
    if name == "miss":
        # the middle body hovers half a millimetre over the box: its pair passes the
        # broadphase and misses between two that hit
        return Case(assets, [[s8], [s5], [s4]], TILTS, gap_columns=(1,))
    if name == "big-between":
        return Case(assets, [[s8], [mesh_shape("big", big)], [s5]], TILTS)
    if name == "box-between":
        return Case(assets, [[s8], [box_shape()], [s5]], TILTS)
    if name == "alone":
        # one small pair and a pair multiccd_x does not take (20 vertices): the path of a pair on its own
        return Case(assets, [[s8, mesh_shape("m20", m20)]], TILTS)
    raise KeyError(name)


# case -> the least number of eligible pairs hitting in the unrotated state's first step
MULTI = {"x2": 2, "x3": 3, "x4": 4, "x8": 8, "stack": 4, "flat": 2, "round": 3, "miss": 2, "big-between": 2,
         "box-between": 2}
CASES = list(MULTI) + ["alone"]


def test_small_hulls_keep_every_vertex():
    cm = case("x4").cm
    for n in (4, 5, 8):
        assert n in cm.hull_vertnum.tolist()
    assert (np.asarray(cm.hull_vertnum)[np.asarray(cm.geom_hullid)[:1]] == 8).all()     # the floor box


@pytest.mark.parametrize("name", CASES)
def test_oracle_stays_inside_the_capacity(name):
    """no case is silently capped: the oracle's contacts and rows stay inside
    the capacity the parity tests run at, and every body that starts inside
    another one has a contact in every state"""
    c = case(name)
    st = c.oracle["stats"]
    assert (st[:, 2] == 0).all(), st
    assert (st[:, 0] < NCON).all() and (st[:, 1] < c.rows()).all(), st
    assert (st[:, 0] >= c.nbody - len(c.gap_columns)).all(), st


@pytest.mark.parametrize("name", list(MULTI))
def test_eligible_pairs_hit_in_one_step(name):
    """from the oracle's contacts: at least two eligible pairs hit in the same
    step (the unrotated state; the count each case is built for)"""
    c = case(name)
    el = c.eligible_pairs()
    hit = [t for t in c.touching(None) if t in el]
    assert len(hit) >= 2 and len(hit) >= MULTI[name], (name, hit, el)
    if name == "x8":
        assert len(hit) > 4
    if name == "miss":
        # the hovering body's pair is eligible and has no contact
        missed = [t for t in el if 0 in t and t not in hit]
        assert len(hit) == 2 and len(missed) == 1, (hit, missed)


def test_alone_has_one_eligible_pair():
    c = case("alone")
    el = c.eligible_pairs()
    for t in c.tilts:
        assert len([x for x in c.touching(t) if x in el]) <= 1
    assert len([x for x in c.touching(None) if x in el]) == 1


def test_between_cases_order():
    """the pair that multiccd_x does not take lies between two it takes, in pair order"""
    from mgs.core import mjcf
    for name, want in (("big-between", mjcf.PAIR_CONVEX), ("box-between", mjcf.PAIR_BOXBOX)):
        c = case(name)
        cm = c.cm
        g1, g2, kind = cm.pair_table(cm.ccd_mode())
        order = [tuple(sorted((int(a), int(b)))) for a, b in zip(g1, g2)]
        el = c.eligible_pairs()
        touch = sorted(c.touching(None), key=order.index)
        flags = [t in el for t in touch]
        assert flags == [True, False, True], (name, touch, flags)
        assert int(kind[order.index(touch[1])]) == want


def test_round_pair_is_convex_with_radius():
    from mgs.core import mjcf
    c = case("round")
    cm = c.cm
    g1, g2, kind = cm.pair_table(cm.ccd_mode())
    cap = int(np.nonzero(np.asarray(cm.geom_type) == mjcf.GEOM_TYPES["capsule"])[0][0])
    assert cm.geom_radius[cap] > 0.0
    el = c.eligible_pairs()
    mine = [t for t in c.touching(None) if cap in t]
    assert mine and all(t in el for t in mine), (mine, el)


def test_flat_box_ties_out_of_lane_order():
    """the tapered box lies flat and unrotated: for the direction (0, 0, -1) of
    its own frame its four bottom vertices tie bit for bit, in the expression
    the kernels and the oracle use; lane li of a quad holds vertices li and
    li + 4, and the tied set has indices i < j with j % 4 < i % 4 -- the lowest
    tied lane does not hold the first tied index.  The same holds for the two
    vertices that tie for a direction without an x component (the perturbed
    MPRs about the x axis)."""
    c = case("flat")
    cm = c.cm
    V8 = taper_points()
    # (the mesh frame is the input's moved to the centre of mass: x and y as given)
    hs = [h for h in range(len(cm.hull_vertnum)) if cm.hull_vertnum[h] == 8 and np.allclose(
        np.sort(np.asarray(cm.hull_vert[cm.hull_vertadr[h]:cm.hull_vertadr[h] + 8])[:, :2], 0),
        np.sort(V8[:, :2], 0), atol=1e-9)]
    assert len(hs) == 1
    h = hs[0]
    g = int(np.nonzero(np.asarray(cm.geom_hullid) == h)[0][0])
    assert np.array_equal(np.asarray(cm.geom_quat[g], np.float64), [1.0, 0, 0, 0])
    q0 = c.qpos(None)
    assert np.array_equal(q0[3:7], [1.0, 0, 0, 0])
    V = np.asarray(cm.hull_vert[cm.hull_vertadr[h]:cm.hull_vertadr[h] + 8], np.float64)
    for dl in (np.array([0.0, 0.0, -1.0]), np.array([0.0, -0.01, -1.0]), np.array([0.0, 0.01, -1.0])):
        sc = (V[:, 0] * dl[0] + V[:, 1] * dl[1]) + V[:, 2] * dl[2]
        tied = np.nonzero(sc == sc.max())[0]
        assert len(tied) == (4 if dl[1] == 0.0 else 2), (dl, tied)
        assert any(j % 4 < i % 4 for a, i in enumerate(tied) for j in tied[a + 1:]), tied
        assert tied[0] % 4 != min(t % 4 for t in tied), tied


def _gpu():
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_simulate_gpu_parity(name):
    _gpu()
    from mgs.core.engine import Engine
    c = case(name)
    eng = Engine(c.cm, ncon_max=NCON, nefc_max=c.rows(), specialize=False)
    try:
        assert not eng.specialized()
        g = eng.simulate(c.plan)
    finally:
        eng.close()
    o = c.oracle
    for k in ("qpos", "qvel", "qacc_warmstart", "stats"):
        assert np.array_equal(g[k], o[k]), (name, k)
    assert np.abs(g["qvel"]).max() > 0.0
