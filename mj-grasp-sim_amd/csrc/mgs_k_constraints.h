// mgs_k_constraints.h -- jac_*, impedance, the constraint rows, make_constraints,
// contact_blocks.
#pragma once
#include "mgs_k_base.h"
#include "mgs_k_math.h"
#include "mgs_k_layout.h"
// ---------------------------------------------------------------------------
// constraints
DEVI void jac_point(const Mdl& md, const Dat& d, int b, const double* pt, double* jacp, double* jacr) {
  int nv = md.m.nv;
  for (int k = 0; k < 3 * nv; k++) { jacp[k] = 0.0; jacr[k] = 0.0; }
  int dof = IA(md, body_lastdof)[b];
  const int32_t* dpar = IA(md, dof_parentid);
  const double* c = d.subtree_com + 3 * IA(md, body_rootid)[b];
  double off[3];
  sub3(off, pt, c);
  while (dof >= 0) {
    const double* cd = d.cdof + 6 * dof;
    double cr[3];
    cross3(cr, cd, off);
    for (int k = 0; k < 3; k++) {
      jacr[k * nv + dof] = cd[k];
      jacp[k * nv + dof] = cd[3 + k] + cr[k];
    }
    dof = dpar[dof];
  }
}

// column `col` of the point Jacobian of body b at pt (oracle jac_point(), one
// dof per lane): zero unless dof col moves the body (model body_dofmask).
DEVI void jac_col(const Mdl& md, const Dat& d, int b, const double* pt, int col, double* jp, double* jr) {
  if (dof_moves(md, b, col)) {
    const double* cd = d.cdof + 6 * col;
    const double* c = d.subtree_com + 3 * IA(md, body_rootid)[b];
    double off[3], cr[3];
    sub3(off, pt, c);
    cross3(cr, cd, off);
    for (int k = 0; k < 3; k++) {
      jr[k] = cd[k];
      jp[k] = cd[3 + k] + cr[k];
    }
  } else {
    for (int k = 0; k < 3; k++) { jr[k] = 0.0; jp[k] = 0.0; }
  }
}

DEVI double impedance(const double* si, double pos, double margin) {
  if (si[0] == si[1] || si[2] <= K_MINVAL) return 0.5 * (si[0] + si[1]);
  double x = (pos - margin) / si[2];
  if (x < 0.0) x = -x;
  if (x >= 1.0) return si[1];
  if (x <= 0.0) return si[0];
  int pw = (int)si[4];
  double mid = si[3], y;
  if (pw <= 1) y = x;
  else if (x <= mid) {
    double a = 1.0, xp = 1.0;
    for (int k = 0; k < pw - 1; k++) a = a * mid;
    a = 1.0 / a;
    for (int k = 0; k < pw; k++) xp = xp * x;
    y = a * xp;
  } else {
    double b = 1.0, xp = 1.0;
    for (int k = 0; k < pw - 1; k++) b = b * (1.0 - mid);
    b = 1.0 / b;
    for (int k = 0; k < pw; k++) xp = xp * (1.0 - x);
    y = 1.0 - b * xp;
  }
  return si[0] + y * (si[1] - si[0]);
}

// lane 0 only
DEVI int add_row(const Mdl& md, Dat& d, int type, double pos, double margin, int dim, int con) {
  if (d.NEFC >= md.m.nefc_max) { d.OVERFLOW |= 2; return -1; }
  int r = d.NEFC++;
  d.efc_type[r] = type; d.efc_pos[r] = pos; d.efc_margin[r] = margin;
  d.efc_dim[r] = dim; d.efc_con[r] = con;
  return r;
}

// lane 0 only; ipos: the violation the impedance is taken at (the row's own
// efc_pos, or an equality constraint's violation norm, eq_violation_norm)
DEVI void row_params(const Mdl& md, Dat& d, int r, int dim, const double* sr, const double* si,
                           const double* mu, int elliptic_contact, double ipos) {
  const double dt = md.m.timestep;
  double tc = sr[0], dr = sr[1];
  double imp = impedance(si, ipos, d.efc_margin[r]);
  double dmax = si[1];
  double B, Kc;
  if (tc > 0.0) {
    if (tc < 2.0 * dt) tc = 2.0 * dt;
    B = 2.0 / (dmax * tc);
    Kc = 1.0 / (((dmax * dmax) * (tc * tc)) * (dr * dr));
  } else {
    B = -dr / dmax;
    Kc = -tc / (dmax * dmax);
  }
  for (int j = 0; j < dim; j++) {
    int q = r + j;
    double p = (j == 0) ? (d.efc_pos[q] - d.efc_margin[q]) : 0.0;
    d.efc_aref[q] = -B * d.efc_vel[q] - (Kc * imp) * p;
  }
  double Rn = ((1.0 - imp) / imp) * d.scratch[r];
  if (Rn < K_MINVAL) Rn = K_MINVAL;
  d.efc_R[r] = Rn;
  if (elliptic_contact && dim > 1) {
    double R1 = Rn / md.m.impratio;
    d.efc_R[r + 1] = R1;
    for (int j = 1; j < dim - 1; j++) d.efc_R[r + j + 1] = (R1 * (mu[0] * mu[0])) / (mu[j] * mu[j]);
  } else {
    for (int j = 1; j < dim; j++) {
      double Rj = ((1.0 - imp) / imp) * d.scratch[r + j];
      d.efc_R[r + j] = Rj < K_MINVAL ? K_MINVAL : Rj;
    }
  }
}

// the norm of an equality constraint's violation over all of its rows (a
// connect's 3, a weld's 6, a joint equality's 1), summed in row order: the
// impedance of every row of the constraint is taken at it (oracle
// eq_violation_norm; round 5, the choice that reproduces MuJoCo's recorded
// Robotiq state_close)
DEVI double eq_violation_norm(const Dat& d, int r) {
  const int id = d.efc_con[r];
  int q = r;
  while (q > 0 && d.efc_type[q - 1] == MGS_EFC_EQUALITY && d.efc_con[q - 1] == id) q--;
  double s2 = 0.0;
  for (; d.efc_type[q] == MGS_EFC_EQUALITY && d.efc_con[q] == id; q++) {
    s2 = s2 + d.efc_pos[q] * d.efc_pos[q];
    if (q + 1 >= d.NEFC) break;
  }
  return sqrt(s2);
}

// MuJoCo mj_diagApprox from the qpos0 inverse weights (oracle diag_approx()); lane 0
DEVI void diag_approx_row(const Mdl& md, Dat& d, int r) {
  const double *biw = DA(md, body_invweight0), *diw = DA(md, dof_invweight0);
  const int32_t *et = IA(md, eq_type), *eo1 = IA(md, eq_obj1id), *eo2 = IA(md, eq_obj2id);
  const int32_t *jd = IA(md, jnt_dofadr), *gbody = IA(md, geom_bodyid);
  int t = d.efc_type[r], id = d.efc_con[r];
  int start = r;
  while (start > 0 && d.efc_type[start - 1] == t && d.efc_con[start - 1] == id) start--;
  int k = r - start;
  double v = 0.0;
  if (t == MGS_EFC_EQUALITY) {
    if (et[id] == MGS_EQ_CONNECT) v = biw[2 * eo1[id]] + biw[2 * eo2[id]];
    else if (et[id] == MGS_EQ_WELD) v = biw[2 * eo1[id] + (k > 2)] + biw[2 * eo2[id] + (k > 2)];
    else {
      v = diw[jd[eo1[id]]];
      if (eo2[id] >= 0) v = v + diw[jd[eo2[id]]];
    }
  } else if (t == MGS_EFC_FRICTION) {
    v = diw[id];
  } else if (t == MGS_EFC_LIMIT) {
    v = diw[jd[id]];
  } else {
    int b1 = gbody[d.con_g1[id]], b2 = gbody[d.con_g2[id]];
    v = (k < 3) ? biw[2 * b1] + biw[2 * b2] : biw[2 * b1 + 1] + biw[2 * b2 + 1];
  }
  d.scratch[r] = v;   // efc_diagApprox, consumed by row_params
}

// Build J rows (into the G slots), then per row: velocity, J.qacc_smooth,
// whitened row G = D^-1/2 L^-1 J^T in place, A = G.G; impedance; blocks.
template <int NV>
DEVI void make_constraints(const Mdl& md, Dat& d) {
  int nv = md.m.nv, lane = lane_id();
  int* ints = d.ints;
  double* J = d.G;
  if (lane == 0) { d.NEFC = 0; }
  wsync();
  const int32_t *et = IA(md, eq_type), *eo1 = IA(md, eq_obj1id), *eo2 = IA(md, eq_obj2id);
  const double* ed = DA(md, eq_data);
  if (md.m.neq <= WAVE) {
    // every equality at once.  Lane e: its rows' place (connect 3, weld 6,
    // joint 1, in equality order) and values; the kept set is the oracle's
    // (make_constraints): equalities before the first one whose rows do not
    // fit, which flags the overflow.  Then lanes over (equality, dof) fill the
    // J columns with the sequential expressions.
    const int neq = md.m.neq;
    const int32_t *jqa = IA(md, jnt_qposadr), *jda = IA(md, jnt_dofadr);
    int typ = -1, need = 0;
    if (lane < neq) {
      typ = et[lane];
      need = typ == MGS_EQ_CONNECT ? 3 : typ == MGS_EQ_WELD ? 6 : typ == MGS_EQ_JOINT ? 1 : 0;
    }
    int re = 0;
    for (int j = 0; j < neq; j++) {
      int nj = __builtin_amdgcn_readlane(need, j);
      if (j < lane) re += nj;
    }
    unsigned long long mbad = __ballot(need > 0 && re + need > md.m.nefc_max);
    int ebad = mbad ? __ffsll((long long)mbad) - 1 : neq;
    int nkeep = ebad;
    if (lane < nkeep && need > 0) {
      const double* data = ed + 11 * lane;
      if (typ == MGS_EQ_JOINT) {
        int j1 = eo1[lane], j2 = eo2[lane];
        double q1 = d.qpos[jqa[j1]] - data[5];
        double pos;
        if (j2 >= 0) {
          double x = d.qpos[jqa[j2]] - data[6];
          double poly = data[0] + x * (data[1] + x * (data[2] + x * (data[3] + x * data[4])));
          pos = q1 - poly;
        } else {
          pos = q1 - data[0];
        }
        d.efc_type[re] = MGS_EFC_EQUALITY; d.efc_pos[re] = pos; d.efc_margin[re] = 0.0;
        d.efc_dim[re] = 1; d.efc_con[re] = lane;
      } else {
        int b1 = eo1[lane], b2 = eo2[lane];
        double p1[3], p2[3], t[3];
        mulmv3(t, d.xmat + 9 * b1, data);
        add3(p1, d.xpos + 3 * b1, t);
        if (typ == MGS_EQ_CONNECT) {
          mulmv3(t, d.xmat + 9 * b2, data + 3);
          add3(p2, d.xpos + 3 * b2, t);
        } else {
          p2[0] = d.xpos[3 * b2]; p2[1] = d.xpos[3 * b2 + 1]; p2[2] = d.xpos[3 * b2 + 2];
        }
        for (int k = 0; k < 3; k++) {
          d.efc_type[re + k] = MGS_EFC_EQUALITY; d.efc_pos[re + k] = p1[k] - p2[k]; d.efc_margin[re + k] = 0.0;
          d.efc_dim[re + k] = 1; d.efc_con[re + k] = lane;
        }
        if (typ == MGS_EQ_WELD) {
          double q1r[4], q2c[4], qe[4];
          quatmul(q1r, d.xquat + 4 * b1, data + 3);
          q2c[0] = d.xquat[4 * b2]; q2c[1] = -d.xquat[4 * b2 + 1];
          q2c[2] = -d.xquat[4 * b2 + 2]; q2c[3] = -d.xquat[4 * b2 + 3];
          quatmul(qe, q2c, q1r);
          double ts = data[7];
          for (int k = 0; k < 3; k++) {
            d.efc_type[re + 3 + k] = MGS_EFC_EQUALITY; d.efc_pos[re + 3 + k] = qe[1 + k] * ts;
            d.efc_margin[re + 3 + k] = 0.0; d.efc_dim[re + 3 + k] = 1; d.efc_con[re + 3 + k] = lane;
          }
        }
      }
    }
    int last = nkeep > 0 ? nkeep - 1 : 0;
    int ne_eq = nkeep > 0 ? __builtin_amdgcn_readlane(re + need, last) : 0;
    for (int q0 = 0; q0 < nkeep * nv; q0 += WAVE) {
      int q = q0 + lane;
      int e = q / nv, col = q - e * nv;
      int es = e < nkeep ? e : nkeep - 1;
      int r = shfl(re, es), ty = shfl(typ, es);
      if (q < nkeep * nv && ty >= 0) {
        const double* data = ed + 11 * e;
        if (ty == MGS_EQ_JOINT) {
          int j1 = eo1[e], j2 = eo2[e];
          double v = (col == jda[j1]) ? 1.0 : 0.0;
          if (j2 >= 0 && col == jda[j2]) {
            double x = d.qpos[jqa[j2]] - data[6];
            double deriv = data[1] + x * (2.0 * data[2] + x * (3.0 * data[3] + x * (4.0 * data[4])));
            v = v - deriv;
          }
          J[r * d.gs + col] = v;
        } else if (ty == MGS_EQ_CONNECT || ty == MGS_EQ_WELD) {
          int b1 = eo1[e], b2 = eo2[e];
          double p1[3], p2[3], t[3];
          mulmv3(t, d.xmat + 9 * b1, data);
          add3(p1, d.xpos + 3 * b1, t);
          if (ty == MGS_EQ_CONNECT) {
            mulmv3(t, d.xmat + 9 * b2, data + 3);
            add3(p2, d.xpos + 3 * b2, t);
          } else {
            p2[0] = d.xpos[3 * b2]; p2[1] = d.xpos[3 * b2 + 1]; p2[2] = d.xpos[3 * b2 + 2];
          }
          double cjp1[3], cjr1[3], cjp2[3], cjr2[3];
          jac_col(md, d, b1, p1, col, cjp1, cjr1);
          jac_col(md, d, b2, p2, col, cjp2, cjr2);
          for (int k = 0; k < 3; k++) J[(r + k) * d.gs + col] = cjp1[k] - cjp2[k];
          if (ty == MGS_EQ_WELD) {
            double q1r[4], q2c[4];
            quatmul(q1r, d.xquat + 4 * b1, data + 3);
            q2c[0] = d.xquat[4 * b2]; q2c[1] = -d.xquat[4 * b2 + 1];
            q2c[2] = -d.xquat[4 * b2 + 2]; q2c[3] = -d.xquat[4 * b2 + 3];
            double ts = data[7];
            double ax[4] = {0.0, cjr1[0] - cjr2[0], cjr1[1] - cjr2[1], cjr1[2] - cjr2[2]};
            double t1q[4], t2q[4];
            quatmul(t1q, q2c, ax);
            quatmul(t2q, t1q, q1r);
            for (int k = 0; k < 3; k++) J[(r + 3 + k) * d.gs + col] = (0.5 * t2q[1 + k]) * ts;
          }
        }
      }
    }
    wsync();
    if (lane == 0) {
      d.NEFC = ne_eq;
      if (ebad < neq) d.OVERFLOW |= 2;
    }
    wsync();
  } else
  for (int e = 0; e < md.m.neq; e++) {
    const double* data = ed + 11 * e;
    if (et[e] == MGS_EQ_CONNECT || et[e] == MGS_EQ_WELD) {
      int b1 = eo1[e], b2 = eo2[e];
      double p1[3], p2[3], t[3];
      if (et[e] == MGS_EQ_CONNECT) {
        mulmv3(t, d.xmat + 9 * b1, data);
        add3(p1, d.xpos + 3 * b1, t);
        mulmv3(t, d.xmat + 9 * b2, data + 3);
        add3(p2, d.xpos + 3 * b2, t);
      } else {
        mulmv3(t, d.xmat + 9 * b1, data);
        add3(p1, d.xpos + 3 * b1, t);
        p2[0] = d.xpos[3 * b2]; p2[1] = d.xpos[3 * b2 + 1]; p2[2] = d.xpos[3 * b2 + 2];
      }
      // this equality's rows do not fit: flag and stop (the oracle's rule; a
      // flag left from an earlier step does not stop the loop)
      if (uni(d.NEFC) + (et[e] == MGS_EQ_WELD ? 6 : 3) > md.m.nefc_max) {
        if (lane == 0) d.OVERFLOW |= 2;
        break;
      }
      if (lane == 0)
        for (int k = 0; k < 3; k++) add_row(md, d, MGS_EFC_EQUALITY, p1[k] - p2[k], 0.0, 1, e);
      wsync();
      int r0 = d.NEFC - 3;
      double cjp1[MGS_DPL][3], cjr1[MGS_DPL][3], cjp2[MGS_DPL][3], cjr2[MGS_DPL][3];
#pragma unroll
      for (int h = 0; h < MGS_DPL; h++) {
        const int i = lane + h * WAVE;
        int col = i < nv ? i : 0;
        jac_col(md, d, b1, p1, col, cjp1[h], cjr1[h]);
        jac_col(md, d, b2, p2, col, cjp2[h], cjr2[h]);
        if (i < nv)
          for (int k = 0; k < 3; k++) J[(r0 + k) * d.gs + i] = cjp1[h][k] - cjp2[h][k];
      }
      if (et[e] == MGS_EQ_WELD) {
        double q1r[4], q2c[4], qe[4];
        quatmul(q1r, d.xquat + 4 * b1, data + 3);
        q2c[0] = d.xquat[4 * b2]; q2c[1] = -d.xquat[4 * b2 + 1];
        q2c[2] = -d.xquat[4 * b2 + 2]; q2c[3] = -d.xquat[4 * b2 + 3];
        quatmul(qe, q2c, q1r);
        double ts = data[7];
        wsync();
        if (lane == 0)
          for (int k = 0; k < 3; k++) add_row(md, d, MGS_EFC_EQUALITY, qe[1 + k] * ts, 0.0, 1, e);
        wsync();
        int rr = d.NEFC - 3;
#pragma unroll
        for (int h = 0; h < MGS_DPL; h++) {
          const int i = lane + h * WAVE;
          if (i < nv) {
            double ax[4] = {0.0, cjr1[h][0] - cjr2[h][0], cjr1[h][1] - cjr2[h][1], cjr1[h][2] - cjr2[h][2]};
            double t1q[4], t2q[4];
            quatmul(t1q, q2c, ax);
            quatmul(t2q, t1q, q1r);
            for (int k = 0; k < 3; k++) J[(rr + k) * d.gs + i] = (0.5 * t2q[1 + k]) * ts;
          }
        }
      }
      wsync();
    } else if (et[e] == MGS_EQ_JOINT) {
      int j1 = eo1[e], j2 = eo2[e];
      const int32_t *jq = IA(md, jnt_qposadr), *jd = IA(md, jnt_dofadr);
      double q1 = d.qpos[jq[j1]] - data[5];
      double pos, deriv = 0.0;
      if (j2 >= 0) {
        double x = d.qpos[jq[j2]] - data[6];
        double poly = data[0] + x * (data[1] + x * (data[2] + x * (data[3] + x * data[4])));
        deriv = data[1] + x * (2.0 * data[2] + x * (3.0 * data[3] + x * (4.0 * data[4])));
        pos = q1 - poly;
      } else {
        pos = q1 - data[0];
      }
      if (uni(d.NEFC) + 1 > md.m.nefc_max) {
        if (lane == 0) d.OVERFLOW |= 2;
        break;
      }
      if (lane == 0) add_row(md, d, MGS_EFC_EQUALITY, pos, 0.0, 1, e);
      wsync();
      int r = d.NEFC - 1;
      for (int c = lane; c < nv; c += WAVE) J[r * d.gs + c] = 0.0;
      wsync();
      if (lane == 0) {
        J[r * d.gs + jd[j1]] = 1.0;
        if (j2 >= 0) J[r * d.gs + jd[j2]] = J[r * d.gs + jd[j2]] - deriv;
      }
      wsync();
    }
  }
  PT(31);
  // dof friction-loss rows, then joint-limit rows (lower bound before upper),
  // in the oracle's order: lanes over dofs / joints, ballot prefixes place the
  // rows, rows past nefc_max are dropped with the overflow flag (add_row)
  {
    int ne0 = uni(d.NEFC);
    const double* floss = DA(md, dof_frictionloss);
    unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (WAVE - lane));
    // friction rows in dof order: slot h's rows follow the lower slots' rows
    int hasf[MGS_DPL], rf[MGS_DPL];
    int nf = 0;
#pragma unroll
    for (int h = 0; h < MGS_DPL; h++) {
      const int i = lane + h * WAVE;
      hasf[h] = (i < nv) && floss[i] > 0.0;
      unsigned long long mf = __ballot(hasf[h]);
      rf[h] = ne0 + nf + __popcll(mf & lt);
      nf += __popcll(mf);
      if (hasf[h] && rf[h] < md.m.nefc_max) {
        d.efc_type[rf[h]] = MGS_EFC_FRICTION; d.efc_pos[rf[h]] = 0.0; d.efc_margin[rf[h]] = 0.0;
        d.efc_dim[rf[h]] = 1; d.efc_con[rf[h]] = i;
      }
    }
    int ne1 = ne0 + nf;
    if (ne1 > md.m.nefc_max) ne1 = md.m.nefc_max;
    const int32_t *lim = IA(md, jnt_limited), *jq = IA(md, jnt_qposadr), *jd = IA(md, jnt_dofadr);
    const double *range = DA(md, jnt_range), *jmargin = DA(md, jnt_margin);
    int lo = 0, hi = 0;
    double dlo = 0.0, dhi = 0.0, jm = 0.0;
    if (lane < md.m.njnt && lim[lane]) {
      double q = d.qpos[jq[lane]];
      dlo = q - range[2 * lane];
      dhi = range[2 * lane + 1] - q;
      jm = jmargin[lane];
      lo = dlo < jm;
      hi = dhi < jm;
    }
    unsigned long long ml = __ballot(lo), mh = __ballot(hi);
    int nl = __popcll(ml) + __popcll(mh);
    int rl = ne1 + __popcll(ml & lt) + __popcll(mh & lt);
    int rh = rl + lo;
    if (lo && rl < md.m.nefc_max) {
      d.efc_type[rl] = MGS_EFC_LIMIT; d.efc_pos[rl] = dlo; d.efc_margin[rl] = jm; d.efc_dim[rl] = 1; d.efc_con[rl] = lane;
    }
    if (hi && rh < md.m.nefc_max) {
      d.efc_type[rh] = MGS_EFC_LIMIT; d.efc_pos[rh] = dhi; d.efc_margin[rh] = jm; d.efc_dim[rh] = 1; d.efc_con[rh] = lane;
    }
    int ne2 = ne1 + nl;
    int ovf = ne0 + nf > md.m.nefc_max || ne2 > md.m.nefc_max;
    if (ne2 > md.m.nefc_max) ne2 = md.m.nefc_max;
    // J rows [ne0, ne2): zeros, then the unit entries
    for (int e = lane; e < (ne2 - ne0) * GS; e += WAVE) J[ne0 * GS + e] = 0.0;
    wsync();
#pragma unroll
    for (int h = 0; h < MGS_DPL; h++)
      if (hasf[h] && rf[h] < md.m.nefc_max) J[rf[h] * GS + lane + h * WAVE] = 1.0;
    if (lo && rl < md.m.nefc_max) J[rl * GS + jd[lane]] = 1.0;
    if (hi && rh < md.m.nefc_max) J[rh * GS + jd[lane]] = -1.0;
    if (lane == 0) {
      ints[8] = ne0; ints[9] = ne0; ints[10] = ne1; ints[11] = ne1; ints[12] = ne2; ints[6] = ne2;
      d.NEFC = ne2;
      if (ovf) d.OVERFLOW |= 2;
    }
  }
  wsync();
  PT(32);
  const int32_t *gbody = IA(md, geom_bodyid), *pcd = IA(md, pair_condim);
  const double *pfr = DA(md, pair_friction), *pmar = DA(md, pair_margin);
  // contact rows, every contact at once: lane c places contact c's dim rows
  // after the rows of contacts 0..c-1 (the sequential order); contacts from
  // the first one that does not fit on are dropped with the overflow flag (the
  // sequential loop stops there).  Then lanes over (contact, dof) pairs fill
  // the J columns.
  int ncon = uni(d.NCON);
  if (ncon > WAVE) {
    // more contacts than lanes (wide capacities): one contact at a time
    for (int c = 0; c < ncon; c++) {
      int p = uni(d.con_pair[c]);
      int dim = pcd[p];
      if (d.NEFC + dim > md.m.nefc_max) {
        if (lane == 0) d.OVERFLOW |= 2;
        break;
      }
      int b1 = gbody[d.con_g1[c]], b2 = gbody[d.con_g2[c]];
      const double* pt = d.con_pos + 3 * c;
      const double* fr = d.con_frame + 9 * c;
      int r = d.NEFC;
      wsync();
      if (lane == 0) {
        for (int j = 0; j < dim; j++) add_row(md, d, MGS_EFC_CONTACT, j == 0 ? d.con_dist[c] : 0.0, pmar[p], dim, c);
        for (int j = 0; j < dim; j++)
          if (!MGS_MU_MODEL && (MGS_MAXDIM < 6 || j < 5)) d.con_mu[5 * c + j] = (j < dim - 1) ? pfr[5 * p + j] : 0.0;
      }
      wsync();
#pragma unroll
      for (int h = 0; h < MGS_DPL; h++) {
      const int i = lane + h * WAVE;
      int col = i < nv ? i : 0;
      double cjp1[3], cjr1[3], cjp2[3], cjr2[3];
      jac_col(md, d, b1, pt, col, cjp1, cjr1);
      jac_col(md, d, b2, pt, col, cjp2, cjr2);
      if (i < nv) {
        double dp[3] = {cjp2[0] - cjp1[0], cjp2[1] - cjp1[1], cjp2[2] - cjp1[2]};
        for (int j = 0; j < dim && j < 3; j++) J[(r + j) * d.gs + col] = dot3(fr + 3 * j, dp);
        if (dim >= 4) {
          double dr[3] = {cjr2[0] - cjr1[0], cjr2[1] - cjr1[1], cjr2[2] - cjr1[2]};
          J[(r + 3) * d.gs + col] = dot3(fr, dr);
#if MGS_MAXDIM > 4
          if (dim == 6) {
            J[(r + 4) * d.gs + col] = dot3(fr + 3, dr);
            J[(r + 5) * d.gs + col] = dot3(fr + 6, dr);
          }
#endif
        }
      }
      }
    }
  } else {
    const int ne0 = uni(d.NEFC);
    int cp = 0, cdim = 0;
    if (lane < ncon) {
      cp = d.con_pair[lane];
      cdim = pcd[cp];
    }
    int rc = ne0;
    for (int j = 0; j < ncon; j++) {
      int dj = __builtin_amdgcn_readlane(cdim, j);
      if (j < lane) rc += dj;
    }
    int bad = lane < ncon && rc + cdim > md.m.nefc_max;
    unsigned long long mb = __ballot(bad);
    int nkeep = mb ? (__ffsll((long long)mb) - 1) : ncon;
    if (lane < nkeep) {
      for (int j = 0; j < cdim; j++) {
        int r = rc + j;
        d.efc_type[r] = MGS_EFC_CONTACT; d.efc_pos[r] = j == 0 ? d.con_dist[lane] : 0.0;
        d.efc_margin[r] = pmar[cp]; d.efc_dim[r] = cdim; d.efc_con[r] = lane;
        // (5 friction coefficients per contact: a condim-6 block's sixth row has
        // no slot -- writing one would clobber the next contact's first)
        if (!MGS_MU_MODEL && (MGS_MAXDIM < 6 || j < 5))
          d.con_mu[5 * lane + j] = (j < cdim - 1) ? pfr[5 * cp + j] : 0.0;
      }
    }
    int last = nkeep > 0 ? nkeep - 1 : 0;
    int ne_end = nkeep > 0 ? __builtin_amdgcn_readlane(rc + cdim, last) : ne0;
    for (int q0 = 0; q0 < nkeep * nv; q0 += WAVE) {
      int q = q0 + lane;
      int c = q / nv, col = q - c * nv;
      int cs = c < nkeep ? c : nkeep - 1;
      int r = shfl(rc, cs), dim = shfl(cdim, cs);
      if (q < nkeep * nv) {
        int b1 = gbody[d.con_g1[c]], b2 = gbody[d.con_g2[c]];
        const double* pt = d.con_pos + 3 * c;
        const double* fr = d.con_frame + 9 * c;
        double cjp1[3], cjr1[3], cjp2[3], cjr2[3];
        jac_col(md, d, b1, pt, col, cjp1, cjr1);
        jac_col(md, d, b2, pt, col, cjp2, cjr2);
        double dp[3] = {cjp2[0] - cjp1[0], cjp2[1] - cjp1[1], cjp2[2] - cjp1[2]};
        for (int j = 0; j < dim && j < 3; j++) J[(r + j) * d.gs + col] = dot3(fr + 3 * j, dp);
        if (dim >= 4) {
          double dr[3] = {cjr2[0] - cjr1[0], cjr2[1] - cjr1[1], cjr2[2] - cjr1[2]};
          J[(r + 3) * d.gs + col] = dot3(fr, dr);
#if MGS_MAXDIM > 4
          if (dim == 6) {
            J[(r + 4) * d.gs + col] = dot3(fr + 3, dr);
            J[(r + 5) * d.gs + col] = dot3(fr + 6, dr);
          }
#endif
        }
      }
    }
    wsync();
    if (lane == 0) {
      d.NEFC = ne_end;
      if (nkeep < ncon) d.OVERFLOW |= 2;
    }
  }
  wsync();
  if (lane == 0) ints[7] = d.NEFC;
  wsync();
  PT(9);
  int ne = uni(d.NEFC);
  // per row (lanes over rows): vel, J.qacc_smooth, G in place, A
  // (the row lives in registers for the triangular solve)
  for (int r = lane; r < ne; r += WAVE) {
    double* Gr = d.G + r * GS;
    double g[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) g[k] = Gr[k];
    double v = 0.0, bj = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++) v = v + g[k] * d.qvel[k];
#pragma unroll
    for (int k = 0; k < NV; k++) bj = bj + g[k] * d.qacc_smooth[k];
    d.efc_vel[r] = v;
    d.efc_b[r] = bj;
#pragma unroll
    for (int i = 0; i < NV; i++) {
      double s = g[i];
#pragma unroll
      for (int k = 0; k < i; k++) s = __builtin_fma(-d.M[TRI(i, k, NV)], g[k], s);
      g[i] = s;
    }
#pragma unroll
    for (int i = 0; i < NV; i++) Gr[i] = g[i] * d.isD[i];
  }
  wsync();
  PT(10);
  // diagApprox then impedance / reference acceleration, lanes over rows (blocks
  // by their leading row); each lane writes only its own rows
  for (int r = lane; r < ne; r += WAVE) diag_approx_row(md, d, r);
  wsync();
  for (int r = lane; r < ne; r += WAVE) {
    int t = d.efc_type[r], id = d.efc_con[r];
    if (t == MGS_EFC_EQUALITY) {
      row_params(md, d, r, 1, DA(md, eq_solref) + 2 * id, DA(md, eq_solimp) + 5 * id, nullptr, 0,
                 eq_violation_norm(d, r));
    } else if (t == MGS_EFC_FRICTION) {
      row_params(md, d, r, 1, DA(md, dof_solref) + 2 * id, DA(md, dof_solimp) + 5 * id, nullptr, 0, d.efc_pos[r]);
    } else if (t == MGS_EFC_LIMIT) {
      row_params(md, d, r, 1, DA(md, jnt_solref) + 2 * id, DA(md, jnt_solimp) + 5 * id, nullptr, 0, d.efc_pos[r]);
    } else if (efc_lead(d, r)) {
      int p = d.con_pair[id];
      row_params(md, d, r, d.efc_dim[r], DA(md, pair_solref) + 2 * p, DA(md, pair_solimp) + 5 * p,
                 con_mu_of(md, d, id), 1, d.efc_pos[r]);
    }
  }
  wsync();
  for (int r = lane; r < ne; r += WAVE) d.efc_b[r] = d.efc_b[r] - d.efc_aref[r];
  wsync();
  PT(11);
}

// contact blocks of A = G G^T for the (PGS / noslip) block updates, lanes over
// block entries; they share storage with the Newton cone Hessians
DEVI void contact_blocks(const Mdl& md, Dat& d) {
  int nv = md.m.nv, lane = lane_id();
  int* ints = d.ints;
  for (int r = uni(ints[6]); r < uni(ints[7]);) {
    int dim = uni(d.efc_dim[r]);
    double* blk = d.con_blk + BLKSTRIDE * uni(d.efc_con[r]);
    for (int e = lane; e < dim * dim; e += WAVE) {
      int i = e / dim, j = e % dim;
      const double* Gi = d.G + (r + i) * d.gs;
      const double* Gj = d.G + (r + j) * d.gs;
      double a = 0.0;
      for (int k = 0; k < nv; k++) a = a + Gi[k] * Gj[k];
      blk[i * dim + j] = a;
    }
    r += dim;
  }
  wsync();
}
