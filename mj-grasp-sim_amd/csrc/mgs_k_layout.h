// mgs_k_layout.h -- the LDS layout (L_* / U_* enums, hbm_slice, Lay), the specialised
// model's header (MGS_SPECIAL), bind<SL>, row helpers.
#pragma once
#include "mgs_k_base.h"
// ---------------------------------------------------------------------------
// LDS layout (offsets in doubles; computed on the host by make_layout)
// LDS carve-up (make_layout in mgs_capi.hip).  Persistent arrays live for the
// whole step; the U region is time-multiplexed between stages:
//   kin/collision: polygon buffers, geom poses, xipos/xanchor/xaxis, comPos sums
//   dynamics:      crb | cvel, cacc, cfrc, cdof_dot, qfrc_bias/passive/actuator
//   constraints:   G, aref, {vel,pos,margin | Newton Hessian}, scratch, Newton rows
//   integration:   qDeriv
enum {
  L_qpos, L_qvel, L_qacc_ws, L_ctrl, L_mocap_pos, L_mocap_quat, L_time, L_act, L_act_dot,
  L_xpos, L_xquat, L_xmat, L_subtree_com, L_cinert, L_cdof,
  L_M, L_Dv, L_Dinv, L_sD, L_isD, L_tmp, L_tmp2,
  L_qfrc_smooth, L_qacc_smooth, L_qfrc_constraint,
  L_act_force, L_act_moment, L_act_length, L_act_vel,
  L_con_pos, L_con_frame, L_con_dist, L_con_mu, L_con_blk,
  L_efc_R, L_efc_b, L_cert,
  L_U, L_ints, L_COUNT
};
enum {
  U_poly, U_pdep, U_geom_xpos, U_geom_xmat, U_xipos, U_xanchor, U_xaxis, U_subtree_mass, U_comacc,
  U_crb, U_cvel, U_cacc, U_cfrc, U_cdof_dot, U_qfrc_bias, U_qfrc_passive, U_qfrc_actuator,
  U_G, U_aref, U_vel, U_pos, U_margin, U_nH, U_scratch, U_jar, U_jv, U_f, U_Dr, U_isR, U_nw, U_nw0, U_ng,
  U_ndir, U_qDeriv, U_COUNT
};
// doubles of one candidate's HBM slice (G rows, and with MGS_HBM_EXTRA the
// certificates, contact frames and contact blocks); mgs_capi.hip's hbm_slice
// allocates the same
#ifndef MGS_HBM_EXTRA
#define MGS_HBM_EXTRA 0
#endif
// ... and a copy of the unfactored M for integrate (m_copy_slot), so the step
// computes crb() once.  MGS_M_KEEP 0 recomputes (A/B builds; the slice keeps
// its size: the host sizes it without knowing the object's switch)
#ifndef MGS_M_KEEP
#define MGS_M_KEEP 1
#endif
DEVI size_t hbm_slice(int ne, int nv, int nc) {
  return (size_t)ne * nv +
         (MGS_HBM_EXTRA ? (size_t)(K_CERT * CERT_W + 9 * nc + BLKSTRIDE * nc + TRI_SIZE(nv)) : 0);
}
struct Lay {
  int o[L_COUNT];
  int u[U_COUNT];   // offsets relative to o[L_U]
  int ncon_max, nefc_max, nv;
  int total_doubles;
  double* gmem;     // MGS_G_GLOBAL: per-candidate G rows in HBM (nefc_max * nv doubles each)
};

// Model specialisation: a code object compiled for one model (mgs_special.hip
// with the header mgs.core.special generates for it, -DMGS_SPECIAL=<header>)
// carries that model's LDS carve-up and description as compile-time constants.
// A kernel instantiated with SL = 1 binds every view at a constant LDS address,
// so the ~80 views need no SGPRs (their spills to VGPR lanes and reloads
// disappear), LDS accesses carry their offsets as instruction immediates, and
// sizes / table offsets / options are constants (trip counts, immediates).
// The host attaches such an object to a model only after comparing the
// object's baked description and layout with the model's
// (mgs_model_attach_special).
#ifdef MGS_SPECIAL
#include MGS_SPECIAL
static_assert(MGS_SL_ABI == MGS_ABI_VERSION, "specialisation header of another ABI version: regenerate it");
static_assert(MGS_SL_DESC_BYTES == sizeof(mgs_model_desc), "specialisation header of another mgs_model_desc");
#else
#define MGS_SL_NV 0
constexpr int mgs_sl_words[L_COUNT + U_COUNT + 4] = {0};
constexpr mgs_model_desc mgs_sl_desc = {};
#endif
static_assert(sizeof(mgs_sl_words) == sizeof(int) * (L_COUNT + U_COUNT + 4), "specialised layout size");

template <int SL>
DEVI void bind(Dat& d, double* s, const Lay& l) {
#define LO(k) (SL ? mgs_sl_words[k] : l.o[k])
#define LU(k) (SL ? mgs_sl_words[L_COUNT + (k)] : l.u[k])
#define B(f) d.f = s + LO(L_##f)
  B(qpos); B(qvel); B(qacc_ws); B(ctrl); B(mocap_pos); B(mocap_quat); B(time); B(act); B(act_dot);
  B(xpos); B(xquat); B(xmat); B(subtree_com); B(cinert); B(cdof);
  B(M); B(Dv); B(Dinv); B(sD); B(isD); B(tmp); B(tmp2);
  B(qfrc_smooth); B(qacc_smooth); B(qfrc_constraint);
  B(act_force); B(act_moment); B(act_length); B(act_vel);
  B(con_pos); B(con_frame); B(con_dist); B(con_mu); B(con_blk);
  B(efc_R); B(efc_b); B(cert);
#undef B
  double* U = s + LO(L_U);
#define BU(f, k) d.f = U + LU(k)
  d.poly = (P2*)(U + LU(U_poly));
  BU(pdep, U_pdep); BU(geom_xpos, U_geom_xpos); BU(geom_xmat, U_geom_xmat); BU(xipos, U_xipos);
  BU(xanchor, U_xanchor); BU(xaxis, U_xaxis); BU(subtree_mass, U_subtree_mass); BU(comacc, U_comacc);
  BU(crb, U_crb); BU(cvel, U_cvel); BU(cacc, U_cacc); BU(cfrc, U_cfrc); BU(cdof_dot, U_cdof_dot);
  BU(qfrc_bias, U_qfrc_bias); BU(qfrc_passive, U_qfrc_passive); BU(qfrc_actuator, U_qfrc_actuator);
#ifdef MGS_G_GLOBAL
  // wide library (clutter piles): G = D^-1/2 L^-1 J' is too large for LDS at
  // nefc_max 256 x nv 58; it lives in this candidate's HBM slice (L2-cached).
  // Main-library objects with G in HBM (MGS_HBM_EXTRA) keep the separation
  // certificates, the contact frames and the contact blocks there too.
  {
    const int sl_nc = SL ? mgs_sl_words[L_COUNT + U_COUNT] : l.ncon_max;
    const int sl_ne = SL ? mgs_sl_words[L_COUNT + U_COUNT + 1] : l.nefc_max;
    const int sl_nv = SL ? mgs_sl_words[L_COUNT + U_COUNT + 2] : l.nv;
    d.G = l.gmem + (size_t)blockIdx.x * hbm_slice(sl_ne, sl_nv, sl_nc);
#if MGS_HBM_EXTRA
    double* x = d.G + (size_t)sl_ne * sl_nv;
    d.cert = x;
    x += K_CERT * CERT_W;
    d.con_frame = x;
    x += 9 * sl_nc;
    d.con_blk = x;
#endif
  }
#else
  BU(G, U_G);
#endif
  BU(efc_aref, U_aref); BU(efc_vel, U_vel); BU(efc_pos, U_pos); BU(efc_margin, U_margin);
  BU(nH, U_nH); BU(scratch, U_scratch); BU(efc_jar, U_jar); BU(efc_jv, U_jv); BU(efc_f, U_f);
  BU(efc_Dr, U_Dr); BU(efc_isR, U_isR); BU(nw, U_nw); BU(nw0, U_nw0); BU(ng, U_ng); BU(ndir, U_ndir);
  BU(qDeriv, U_qDeriv);
#undef BU
  d.con_hb = d.con_blk;   // Newton cone Hessians reuse the contact-block slots
  d.gs = (SL ? mgs_sl_words[L_COUNT + U_COUNT + 2] : l.nv) + MGS_GPAD;
  int* ib = (int*)(s + LO(L_ints));
  d.ints = ib;
  int ncmax = SL ? mgs_sl_words[L_COUNT + U_COUNT] : l.ncon_max;
  int nemax = SL ? mgs_sl_words[L_COUNT + U_COUNT + 1] : l.nefc_max;
  d.con_pair = ib + 16;
  d.con_g1 = d.con_pair + ncmax;
  d.con_g2 = d.con_g1 + ncmax;
  d.efc_type = d.con_g2 + ncmax;
  d.efc_dim = d.efc_type + nemax;
  d.efc_con = d.efc_dim + nemax;
  d.efc_state = d.efc_con + nemax;
#undef LO
#undef LU
}

// A_rr = G_r . G_r in the oracle's order (its efc_A)
DEVI double row_sqnorm(const Dat& d, int r, int nv) {
  const double* Gr = d.G + r * d.gs;
  double a = 0.0;
  for (int k = 0; k < nv; k++) a = a + Gr[k] * Gr[k];
  return a;
}

// first row of its block (contacts span dim rows with one efc_con)
DEVI int efc_lead(const Dat& d, int r) {
  return d.efc_type[r] != MGS_EFC_CONTACT || r == 0 || d.efc_type[r - 1] != MGS_EFC_CONTACT ||
         d.efc_con[r - 1] != d.efc_con[r];
}

// contact c's friction coefficients (see MGS_MU_MODEL)
DEVI const double* con_mu_of(const Mdl& md, const Dat& d, int c) {
#if MGS_MU_MODEL
  return DA(md, pair_friction) + 5 * d.con_pair[c];
#else
  (void)md;
  return d.con_mu + 5 * c;
#endif
}

// frictionloss of a FRICTION row (its efc_con is the dof), 0 otherwise
DEVI double row_floss(const Mdl& md, const Dat& d, int r) {
  return d.efc_type[r] == MGS_EFC_FRICTION ? DA(md, dof_frictionloss)[d.efc_con[r]] : 0.0;
}

