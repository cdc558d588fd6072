"""Group-local support mappings of the lockstep MPRs (multiccd's four perturbed
MPRs of a pair with a hull of more than 8 vertices or a cylinder: each 16-lane
group scans the hulls itself, mgs_kernels.hip support_pairg).

Small synthetic models (nv 14, 20 or 28: the generic library's kernels, no code
object is compiled) with the multiccd flag on: a mesh starts a fraction of a
millimetre inside a box, a second body inside the mesh, in several states
each (unrotated, turned at random, resting on a hull face so that multiccd's
tilted MPRs add contacts).  Ten free-simulation steps on the GPU are compared
bit for bit with the oracle's (as tests/test_scene_gen.py does).  Hull sizes on both sides of every path of the
scan (one take from the cached vertex up to 16, batches of 16 x 4 vertices
above; the whole-wave supports of the first MPR change at 64), exact ties on
a k-gon face whose tied vertices sit in lanes out of index order, cylinders,
rounding radii, and rows of bodies whose pairs follow each other in one step.
CPU: the tie structure of the compiled prisms and the oracle's contact counts
against the capacity used."""
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


def sphere_points(n, r=0.03):
    """n points on a sphere (golden-angle spiral): every one is a hull vertex"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return (r * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(np.float32).astype(np.float64)


def prism_points(k):
    """a tall k-gon prism widening upwards (elliptic sections, so the principal
    axes are x, y, z and the mesh frame is the input's): the bottom face z =
    -0.04 is a k-gon whose vertices all tie for the direction (0, 0, -1); the
    wider top ring sorts first in the compiled (lexicographic) vertex order"""
    a = 2.0 * np.pi * (np.arange(k) + 0.25) / k
    ring = np.stack([0.010 * np.cos(a), 0.014 * np.sin(a)], 1)
    bot = np.concatenate([ring, np.full((k, 1), -0.04)], 1)
    top = np.concatenate([1.5 * ring, np.full((k, 1), 0.04)], 1)
    return np.concatenate([bot, top]).astype(np.float32).astype(np.float64)


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


# a shape: (geom xml, points of its convex core in the body frame, rounding radius)
def mesh_shape(name, pts):
    return (f'<geom type="mesh" mesh="{name}"/>', pts, 0.0)


def capsule_shape(r=0.01, h=0.03):
    # lying along x
    c = np.cos(np.pi / 4)
    return (f'<geom type="capsule" size="{r} {h}" quat="{c} 0 {c} 0"/>', np.array([[-h, 0, 0], [h, 0, 0.0]]), r)


def cylinder_shape(r=0.02, h=0.03):
    a = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    ring = np.stack([r * np.cos(a), r * np.sin(a)], 1)
    pts = np.concatenate([np.concatenate([ring, np.full((64, 1), z)], 1) for z in (-h, h)])
    return (f'<geom type="cylinder" size="{r} {h}"/>', pts, 0.0)


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
                    q = face_down_quat(pts) if len(pts) > 8 else np.array([1.0, 0, 0, 0])
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


TILTS = [None, (1, 0.05), (2, 0.3), (3, 1.0), "face"]
SIZES = [9, 16, 17, 64, 65, 186, 256, 257, 530]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("-")
    if kind == "sphere":
        # the n-vertex hull on the box, a 20-vertex hull on top of it (hull-box and hull-hull pairs)
        n = int(arg)
        return Case([mesh_xml("a", sphere_points(n)), mesh_xml("b", sphere_points(20, 0.02))],
                    [[mesh_shape("a", sphere_points(n)), mesh_shape("b", sphere_points(20, 0.02))]], TILTS)
    if kind == "prism":
        # flat and unrotated over the box's centre (state 0: the whole face ties), and tilted
        k = int(arg)
        return Case([mesh_xml("a", prism_points(k)), mesh_xml("b", sphere_points(12, 0.02))],
                    [[mesh_shape("a", prism_points(k)), mesh_shape("b", sphere_points(12, 0.02))]],
                    [None, (4, 1e-3), (5, 0.02)])
    if kind == "round":
        # a cylinder standing on the box with a capsule lying on it (exact cylinder support, rounding radius)
        return Case([], [[cylinder_shape(), capsule_shape()]], [None, (6, 0.02), (7, 0.2)])
    if kind == "capmesh":
        # a capsule lying on a 186-vertex hull
        return Case([mesh_xml("a", sphere_points(186))], [[mesh_shape("a", sphere_points(186)), capsule_shape()]],
                    [None, (8, 0.1), "face"])
    big, small = sphere_points(186), sphere_points(8, 0.02)
    assets = [mesh_xml("big", big), mesh_xml("small", small), mesh_xml("mid", sphere_points(40, 0.025))]
    if name == "row-2":
        # two convex pairs follow each other: a big hull and an 8-vertex one on the box
        return Case(assets, [[mesh_shape("big", big)], [mesh_shape("small", small)]], TILTS)
    if name == "row-3":
        return Case(assets, [[mesh_shape("big", big)], [mesh_shape("small", small)],
                             [mesh_shape("mid", sphere_points(40, 0.025))]], TILTS)
    if name == "row-4":
        return Case(assets, [[mesh_shape("big", big)], [mesh_shape("small", small)],
                             [mesh_shape("mid", sphere_points(40, 0.025))], [cylinder_shape(0.015, 0.02)]], TILTS)
    if name == "row-split":
        # a box-box pair between two convex pairs: the run of convex pairs is split there
        return Case(assets, [[mesh_shape("big", big)], [box_shape()], [mesh_shape("small", small)]], TILTS)
    if name == "row-miss":
        # the middle body hovers half a millimetre over the box: its pair passes the
        # broadphase, misses with a separating direction and is skipped by it on the next steps
        return Case(assets, [[mesh_shape("big", big)], [mesh_shape("mid", sphere_points(40, 0.025))],
                             [mesh_shape("small", small)]], TILTS, gap_columns=(1,))
    raise KeyError(name)


CASES = [f"sphere-{n}" for n in SIZES] + ["prism-12", "prism-40", "round", "capmesh",
                                          "row-2", "row-3", "row-4", "row-split", "row-miss"]


def test_sphere_hulls_keep_every_vertex():
    for n in SIZES:
        cm = case(f"sphere-{n}").cm
        assert n in cm.hull_vertnum.tolist() and 20 in cm.hull_vertnum.tolist()


@pytest.mark.parametrize("k", [12, 40])
def test_prism_face_ties_out_of_lane_order(k):
    """the first MPR direction of the box-prism pair is exactly (0, 0, 1), the
    prism's support direction (0, 0, -1) in its own frame: the k face vertices
    tie bit for bit, in the expression the kernels and the oracle use, and the
    tied set has indices i < j with j % 16 < i % 16 -- in particular the lowest
    tied lane of a 16-lane group does not hold the first tied index"""
    c = case(f"prism-{k}")
    cm = c.cm
    h = int(np.nonzero(cm.hull_vertnum == 2 * k)[0][0])
    g = int(np.nonzero(cm.geom_hullid == h)[0][0])
    V = cm.hull_vert[cm.hull_vertadr[h]:cm.hull_vertadr[h] + 2 * k]
    # the geom frame is the body frame: the unrotated state's support direction is the world's
    assert np.array_equal(np.asarray(cm.geom_quat[g], np.float64), [1.0, 0, 0, 0])
    q0 = c.qpos(None)
    assert q0[0] == 0.0 and q0[1] == 0.0 and np.array_equal(q0[3:7], [1.0, 0, 0, 0])   # centred over the box
    # ccd_mpr's first direction: from the prism's centre (its centre of mass: the
    # mesh frame's origin, within 1e-18 of the body's axis) to the box's, here the
    # origin; the prism (geom 2: MuJoCo orders box before mesh) takes its negative
    c2 = q0[:3] + cm.geom_pos[g]
    dl = -(c2 / np.sqrt(c2 @ c2))
    # the off-axis terms are absorbed: half an ulp of the face's 0.04 is 3.5e-18
    assert dl[2] == -1.0 and np.abs(V[:, :2] @ dl[:2]).max() < 1e-18
    sc = (V[:, 0] * dl[0] + V[:, 1] * dl[1]) + V[:, 2] * dl[2]
    tied = np.nonzero(sc == sc.max())[0]
    assert len(tied) == k
    assert any(j % 16 < i % 16 for a, i in enumerate(tied) for j in tied[a + 1:])
    assert tied[0] % 16 != min(t % 16 for t in tied)


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


def test_row_cases_exercise_consecutive_pairs():
    """the rows put 2, 3 and 4 convex pairs with contacts into one step (each
    column touches the box); the split row has a box-box pair between two
    convex ones, the miss row a convex pair that never touches"""
    from mgs.core import mjcf
    from oracle import oracle as O
    for name, want in (("row-2", 2), ("row-3", 3), ("row-4", 4), ("row-split", 3), ("row-miss", 2)):
        c = case(name)
        cm = c.cm
        om = O.OracleModel(cm, ncon_max=NCON, nefc_max=c.rows())
        n, p, fr, dist, g = om.contacts(c.qpos(None), np.zeros(3), np.array([1.0, 0, 0, 0]), maxc=NCON)
        touching = {tuple(sorted(x)) for x in g.tolist()}
        assert len(touching) == want, (name, touching)
        kinds = {tuple(sorted((int(a), int(b)))): int(k)
                 for a, b, k in zip(cm.pair_geom1, cm.pair_geom2, cm.pair_kind)}
        tk = [kinds[t] for t in sorted(touching, key=lambda t: list(kinds).index(t))]
        if name == "row-split":
            assert tk == [mjcf.PAIR_CONVEX, mjcf.PAIR_BOXBOX, mjcf.PAIR_CONVEX], tk
        else:
            assert all(k == mjcf.PAIR_CONVEX for k in tk), tk


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
