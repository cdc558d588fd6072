// mgs_pose.hip -- the cloud of a scanned gripper at B joint states on the
// MI355X (include/mgs_gpu.h "Posed gripper cloud").  The reference's
// kinematic_pcd_transform (mgs/sampler/kin/base.py:34-77) moves the points of
// joint j's mask by T_j delta_j T_j^-1, chain by chain; for masks that nest
// along the tree that product telescopes to one transform per link,
//   M_i = W_i(theta_b) o W_i(theta_scan)^-1,
//   W_i(theta) = W_parent(i)(theta) o kin_tf[i] o J_i(theta_i),   W_base = identity,
// so a point is moved once, by the link it is fixed to.  Included from
// mgs_capi.hip only, after mgs_contact.hip whose c_qmul / c_qrot / c_compose it
// uses.  f64 without contraction; tests/pose_truth.py restates every expression
// in numpy in the same order of operations.
//
// One workgroup = one grasp b and one group of points:
//   stage 1  lane i < nlink lists its ancestors (root first, in LDS), walks
//            them twice (theta_b, theta_scan), forms M_i with the conjugate as
//            the inverse (unit quaternions: the host normalises), turns it into
//            a 3 x 4 matrix, multiplies by the grasp pose when there is one and
//            leaves it in LDS.  Entry 0 (the base) is the identity or the grasp
//            pose itself, not computed.
//   stage 2  tiles of 256 points: the tile's coordinates come into LDS by one
//            contiguous read, each lane moves one point, the results go back
//            through LDS so that a wave stores one contiguous span (16 bytes
//            per lane between an unaligned head and tail).
// No atomics; plain vector stores only.

#define MGS_POSE_THREADS 256

// J_i(theta): quaternion_from_axis_angle(axis, theta) and direction * theta
// (base.py:62-72); a slide joint (axis of norm 0) takes the identity quaternion
// without the division
DEVI void pose_joint_tf(const double* jt, double th, double* J) {
  const double* a = jt + 3;
  double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  J[0] = 1.0; J[1] = 0.0; J[2] = 0.0; J[3] = 0.0;
  if (n > 0.0) {
    double ax = a[0] / n, ay = a[1] / n, az = a[2] / n;
    double h = th / 2.0, s, c;
    k_sincos(h, &s, &c);
    J[0] = c; J[1] = ax * s; J[2] = ay * s; J[3] = az * s;
  }
  J[4] = jt[0] * th; J[5] = jt[1] * th; J[6] = jt[2] * th;
}

// W_i(theta) along the chain (root first) of `len` links
DEVI void pose_link_tf(const mgs_pose_tree& T, const uint8_t* chain, int len, const double* th, double* W) {
  W[0] = 1.0;
  for (int k = 1; k < 7; k++) W[k] = 0.0;
  for (int s = 0; s < len; s++) {
    const int i = chain[s];
    double A[7], J[7];
    c_compose(A, W, T.kin_tf[i]);
    pose_joint_tf(T.joint_tf[i], th[i], J);
    c_compose(W, A, J);
  }
}

// se3_invert (jax_util.py:115-119): the conjugate, and minus the turned translation
DEVI void pose_invert(double* o, const double* W) {
  double r[3];
  o[0] = W[0]; o[1] = -W[1]; o[2] = -W[2]; o[3] = -W[3];
  c_qrot(r, o, W + 4);
  o[4] = -r[0]; o[5] = -r[1]; o[6] = -r[2];
}

// the tile's results in LDS (n values of T) to out[0 .. n): 16-byte stores from
// the first 16-byte boundary of `out`, single values before and after
template <class T>
DEVI void pose_store_tile(T* __restrict__ out, const T* s_out, int n) {
  constexpr int V = 16 / (int)sizeof(T);
  const int t = threadIdx.x;
  int head = (int)(((16u - (unsigned)((uintptr_t)out & 15u)) & 15u) / sizeof(T));
  if (head > n) head = n;
  const int nvec = (n - head) / V;
  if (t < head) out[t] = s_out[t];
  for (int k = t; k < nvec; k += MGS_POSE_THREADS) {
    const T* s = s_out + head + V * k;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(out + head + V * k) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
      *reinterpret_cast<double2*>(out + head + V * k) = make_double2(s[0], s[1]);
    }
  }
  for (int k = head + V * nvec + t; k < n; k += MGS_POSE_THREADS) out[k] = s_out[k];
}

// grid (ceil(npoint / ppg), nbatch), ppg >= 1 points per group.  The tree
// travels by value in the kernel arguments (3.7 KB): no allocation per launch.
// base: nbatch * 12 (row-major 3 x 4) or null; out_links: nbatch * nlink * 7 or null.
template <class T>
__global__ void __launch_bounds__(MGS_POSE_THREADS)
mgs_pose_cloud_kernel(const mgs_pose_tree K, int npoint, const double* __restrict__ points,
                      const int32_t* __restrict__ point_link, const double* __restrict__ theta,
                      const double* __restrict__ base, T* __restrict__ out, double* __restrict__ out_links, int ppg) {
  __shared__ double s_M[(MGS_POSE_MAXLINK + 1) * 12];
  __shared__ double s_th[2 * MGS_POSE_MAXLINK];
  __shared__ uint8_t s_chain[MGS_POSE_MAXLINK][MGS_POSE_MAXLINK];
  __shared__ double s_in[3 * MGS_POSE_THREADS];
  __shared__ T s_out[3 * MGS_POSE_THREADS];
  const int t = threadIdx.x, nl = K.nlink;
  const size_t b = blockIdx.y;

  // ---- stage 1: the links' matrices
  if (t < nl) { s_th[t] = theta[b * nl + t]; s_th[MGS_POSE_MAXLINK + t] = K.theta_scan[t]; }
  if (t < 12) {
    const double eye = (t == 0 || t == 5 || t == 10) ? 1.0 : 0.0;
    s_M[t] = base ? base[12 * b + t] : eye;
  }
  __syncthreads();
  if (t < nl) {
    uint8_t* ch = s_chain[t];
    int len = 0;
    for (int i = t; i >= 0 && len < MGS_POSE_MAXLINK; i = K.parent[i]) len++;
    int s = len;
    for (int i = t; s > 0; i = K.parent[i]) ch[--s] = (uint8_t)i;
    double Wb[7], Ws[7], Wi[7], M[7], R[9];
    pose_link_tf(K, ch, len, s_th, Wb);
    pose_link_tf(K, ch, len, s_th + MGS_POSE_MAXLINK, Ws);
    pose_invert(Wi, Ws);
    c_compose(M, Wb, Wi);
    quat2mat(R, M);
    double* o = s_M + 12 * (t + 1);
    if (base) {
      const double* G = s_M;      // the grasp pose, rows of 4
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++)
          o[4 * r + c] = (G[4 * r] * R[c] + G[4 * r + 1] * R[3 + c]) + G[4 * r + 2] * R[6 + c];
        o[4 * r + 3] = ((G[4 * r] * M[4] + G[4 * r + 1] * M[5]) + G[4 * r + 2] * M[6]) + G[4 * r + 3];
      }
    } else {
      for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = R[3 * r + c];
        o[4 * r + 3] = M[4 + r];
      }
    }
    if (out_links && blockIdx.x == 0)
      for (int k = 0; k < 7; k++) out_links[(b * nl + t) * 7 + k] = Wb[k];
  }
  __syncthreads();

  // ---- stage 2: the group's points, a tile at a time
  const int p_lo = blockIdx.x * ppg;
  const int p_hi = npoint - p_lo < ppg ? npoint : p_lo + ppg;
  for (int p0 = p_lo; p0 < p_hi; p0 += MGS_POSE_THREADS) {
    const int m = p_hi - p0 < MGS_POSE_THREADS ? p_hi - p0 : MGS_POSE_THREADS;
    const double* src = points + 3 * (size_t)p0;
    for (int k = t; k < 3 * m; k += MGS_POSE_THREADS) s_in[k] = src[k];
    __syncthreads();
    if (t < m) {
      const double x = s_in[3 * t], y = s_in[3 * t + 1], z = s_in[3 * t + 2];
      // the host entry refuses a link outside 0 .. nlink; one that reaches the
      // device entry gives NaN, never a read outside the table
      const int l = point_link[p0 + t];
      const bool ok = l >= 0 && l <= nl;
      const double* M = s_M + 12 * (ok ? l : 0);
      for (int r = 0; r < 3; r++) {
        const double v = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3];
        s_out[3 * t + r] = (T)(ok ? v : NAN);
      }
    }
    __syncthreads();
    pose_store_tile(out + 3 * (b * (size_t)npoint + (size_t)p0), s_out, 3 * m);
  }
}
