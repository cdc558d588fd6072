"""Plain-numpy truths of the posed gripper cloud (csrc/mgs_pose.hip).

pose_kernel     the kernel, expression for expression in float64: the shared
                polynomial sincos of csrc/mgs_k_math.h (plain IEEE arithmetic),
                the quaternion algebra of csrc/mgs_contact.hip, the same
                parenthesisation.  The GPU result must equal it bit for bit.
pose_reference  the reference as written: kinematic_pcd_transform chain by
                chain with similarity_transform and the masked update
                (mgs/sampler/kin/base.py:34-77, kin/jax_util.py:20-131), np.sin /
                np.cos, float64.  Independent of the single-transform form.
"""
import numpy as np


# -- the kernel's arithmetic ---------------------------------------------------------
def k_sincos(x):
    """csrc/mgs_k_math.h k_sincos on a Python float"""
    x = np.float64(x)
    inv_pio2 = np.float64(6.36619772367581382433e-01)
    pio2_1 = np.float64(1.57079632673412561417e+00)
    pio2_1t = np.float64(6.07710050650619224932e-11)
    S = [np.float64(v) for v in (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
                                 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)]
    C = [np.float64(v) for v in (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
                                 -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)]
    kd = x * inv_pio2
    kd = np.floor(kd + 0.5) if kd >= 0.0 else -np.floor(0.5 - kd)
    r = (x - kd * pio2_1) - kd * pio2_1t
    z = r * r
    ps = S[0] + z * (S[1] + z * (S[2] + z * (S[3] + z * (S[4] + z * S[5]))))
    sr = r + (r * z) * ps
    pc = C[0] + z * (C[1] + z * (C[2] + z * (C[3] + z * (C[4] + z * C[5]))))
    cr = (1.0 - 0.5 * z) + (z * z) * pc
    q = int(kd) & 3
    return [(sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr)][q]


def c_qmul(a, b):
    return np.array([((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
                     ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
                     ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
                     ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0]])


def c_qrot(q, v):
    p = np.array([0.0, v[0], v[1], v[2]])
    c = np.array([q[0], -q[1], -q[2], -q[3]])
    return c_qmul(c_qmul(q, p), c)[1:]


def c_compose(A, B):
    return np.concatenate([c_qmul(A[:4], B[:4]), c_qrot(A[:4], B[4:]) + A[4:]])


def joint_tf(jt, th):
    a = jt[3:]
    n = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    J = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    if n > 0.0:
        s, c = k_sincos(th / 2.0)
        J[:4] = [c, (a[0] / n) * s, (a[1] / n) * s, (a[2] / n) * s]
    J[4:] = jt[:3] * th
    return J


def link_tf(tree, i, theta):
    """W_i(theta): the chain of link i, root first"""
    chain = []
    while i >= 0:
        chain.append(i)
        i = int(tree.parent[i])
    W = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for k in reversed(chain):
        W = c_compose(c_compose(W, tree.kin_tf[k]), joint_tf(tree.joint_tf[k], theta[k]))
    return W


def invert(W):
    o = np.array([W[0], -W[1], -W[2], -W[3], 0.0, 0.0, 0.0])
    o[4:] = -c_qrot(o[:4], W[4:])
    return o


def quat2mat(q):
    """csrc/mgs_k_math.h quat2mat, rows"""
    q00, q01, q02, q03 = q[0] * q[0], q[0] * q[1], q[0] * q[2], q[0] * q[3]
    q11, q12, q13 = q[1] * q[1], q[1] * q[2], q[1] * q[3]
    q22, q23, q33 = q[2] * q[2], q[2] * q[3], q[3] * q[3]
    return np.array([[((q00 + q11) - q22) - q33, 2.0 * (q12 - q03), 2.0 * (q13 + q02)],
                     [2.0 * (q12 + q03), ((q00 - q11) + q22) - q33, 2.0 * (q23 - q01)],
                     [2.0 * (q13 - q02), 2.0 * (q23 + q01), ((q00 - q11) - q22) + q33]])


def link_matrices(tree, theta, base=None):
    """((nlink + 1, 3, 4) matrices of one joint state, (nlink, 7) W_i(theta)):
    entry 0 is the identity or `base` (3 x 4) as given"""
    n = len(tree.parent)
    M = np.zeros((n + 1, 3, 4))
    M[0] = np.eye(4)[:3] if base is None else base
    links = np.zeros((n, 7))
    for i in range(n):
        Wb = link_tf(tree, i, theta)
        links[i] = Wb
        T = c_compose(Wb, invert(link_tf(tree, i, tree.theta_scan)))
        R, t = quat2mat(T[:4]), T[4:]
        if base is None:
            M[i + 1, :, :3], M[i + 1, :, 3] = R, t
        else:
            G = base
            for r in range(3):
                for c in range(3):
                    M[i + 1, r, c] = (G[r, 0] * R[0, c] + G[r, 1] * R[1, c]) + G[r, 2] * R[2, c]
                M[i + 1, r, 3] = ((G[r, 0] * t[0] + G[r, 1] * t[1]) + G[r, 2] * t[2]) + G[r, 3]
    return M, links


def pose_kernel(tree, points, link, theta, base=None):
    """(points (B, P, 3) float64, links (B, nlink, 7)) as mgs_pose_cloud_kernel
    computes them; base: (B, 3, 4) / (B, 4, 4) or None"""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    link = np.asarray(link, np.int64).reshape(-1)
    theta = np.asarray(theta, np.float64)
    out = np.zeros((len(theta), len(x), 3))
    links = np.zeros((len(theta), len(tree.parent), 7))
    for b in range(len(theta)):
        G = None if base is None else np.asarray(base, np.float64)[b][:3]
        M, links[b] = link_matrices(tree, theta[b], G)
        m = M[link]                                                    # (P, 3, 4)
        for r in range(3):
            out[b, :, r] = ((m[:, r, 0] * x[:, 0] + m[:, r, 1] * x[:, 1]) + m[:, r, 2] * x[:, 2]) + m[:, r, 3]
    return out, links


# -- the reference as written --------------------------------------------------------
def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _qinv(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _qapply(q, pts):
    """quaternion_apply_jax on (..., 3) points"""
    pts = np.asarray(pts, np.float64)
    flat = pts.reshape(-1, 3)
    out = np.zeros_like(flat)
    for k, p in enumerate(flat):
        out[k] = _qmul(_qmul(q, np.concatenate([[0.0], p])), _qinv(q))[1:]
    return out.reshape(pts.shape)


def _se3_mul(A, B):
    return np.concatenate([_qmul(A[:4], B[:4]), _qapply(A[:4], B[4:]) + A[4:]])


def _se3_inv(T):
    qi = _qinv(T[:4])
    return np.concatenate([qi, -_qapply(qi, T[4:])])


def _similarity(Ts, T):
    return _se3_mul(_se3_mul(Ts, T), _se3_inv(Ts))


def _axis_angle(axis, angle):
    axis = axis / np.linalg.norm(axis)
    s = np.sin(angle / 2.0)
    return np.array([np.cos(angle / 2.0), axis[0] * s, axis[1] * s, axis[2] * s])


def pose_reference(chains, kin_tf, joint_tf_, points, theta, segmentation, base_to_contact=None):
    """kinematic_pcd_transform for one joint vector: chains (the kinematics
    graph), segmentation (ndof, P) bool -- the points joint j moves"""
    pts = np.array(points, np.float64).reshape(-1, 3)
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    for chain in chains:
        cur = ident.copy() if base_to_contact is None else np.asarray(base_to_contact, np.float64)
        delta = ident.copy()
        for index in chain:
            cur = _se3_mul(_se3_mul(cur, delta), kin_tf[index])
            th = theta[index]
            translation = joint_tf_[index][:3] * th
            axis = joint_tf_[index][3:]
            rot = _axis_angle(axis, th) if np.linalg.norm(axis) > 0 else np.array([1.0, 0.0, 0.0, 0.0])
            delta = np.concatenate([rot, translation])
            Ts = _similarity(cur, delta)
            mask = np.asarray(segmentation[index], bool)
            moved = _qapply(Ts[:4], pts) + Ts[4:]
            pts = np.where(mask[:, None], moved, pts)
    return pts
