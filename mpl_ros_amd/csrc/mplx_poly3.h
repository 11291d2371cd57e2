// mplx_poly3.h -- the moving-obstacle (PolyMap) environment in 3-D on the device: env_poly_map<3> / PolyMapUtil<3> /
// collide<3> for a batch of states (poly3_get_succ_kernel: the parity entry) and astar_poly3_kernel, GraphSearch::Astar over
// it with one workgroup per query.  Kept apart from the 2-D environment (mplx_poly_dev.h, whose device code stays as it is).
//
// Restates, operation for operation, the reference's in-tree arithmetic at Dim = 3 (paths relative to the reference repo):
//   mpl_external_planner/include/mpl_external_planner/poly_map_planner/env_poly_map.h:45-73   get_succ, intrinsic cost
//   .../poly_map_planner/poly_map_util.h:52-109                     3-D setBoundingBox (host side), isInside, isFree(pt, t), isFree(pr, t)
//   .../poly_map_planner/primitive_geometry_utils.h:5-173           collide() x 3 (static / linear / nonlinear obstacle)
//   .../poly_map_planner/simple_obstacle.h:6-166                    obstacle classes (inside, poly(t))
// and what those call from the un-vendored submodules as include/mpl_shim states it: Primitive1D p/v/a/j/J,
// validate_primitive, Trajectory::evaluate, solve(), Polyhedron::inside (epsilon 1e-10).  Every sum keeps the reference's
// order over i < Dim (`a += n(i) * cs[i](0)` for i = 0, 1, 2, then `a /= 120`; n.dot(x) as s = 0, s += n0 x0, s += n1 x1,
// s += n2 x2); polynomials are always evaluated in their full form (no short forms), so results are bit-identical to the
// host evaluation.  Compiled -ffp-contract=off like the rest.
//
// Shared unchanged with the 2-D environment: pp_p / pp_v / pp_a / pp_j / pp_J, solve_le2 / solve_any6 / solve_poly<GEN>,
// poly_max_abs (mplx_poly_dev.h); the search machinery of mplx_kernels.h (Smem, QView, pools, table, heuristics,
// commit_parallel) and the per-query steps of mplx_search_steps.h.  GEN = false: hyperplane equations of degree <= 2 (ACC primitives among
// static / linear obstacles and obstacles on VEL / ACC trajectories); a higher degree is reported, never approximated.
// GEN = true: any degree up to five through solve_any6 (JRK primitives, obstacle trajectories with cubic or higher segments).
//
// Kernel shape: lane i < n_u builds primitive i (end state, bounding box, validate_primitive, cost, key); the lanes then
// run the start-point test isFree(start.pos, t) over the obstacles and, unless it failed, isFree(pr, t) over the
// (primitive, obstacle) pairs -- one serial collide() each, the reference's loops as they are -- OR-ed in LDS.
#pragma once
#include "mplx_kernels.h"
#include "mplx_poly_dev.h"

namespace mplx {

constexpr int POLY3_MAX_U = 32;

struct Poly3HP { double p[3], n[3]; };                // Hyperplane3D: point p_, outward normal n_
struct Poly3Seg { double c[3][6]; double T; };        // Primitive3D of an obstacle trajectory
struct Poly3Obs {
  int32_t kind;                                       // 0 static, 1 linear, 2 nonlinear
  int32_t hp_off, n_hp, seg_off, n_seg, dis_front, dis_back, pad;
  double p[3], v[3], cov_v, start_t, total_t;         // representative point, velocity (linear), trajectory start / length
};
struct Poly3World {                                   // what one planner sees: bounding box + obstacle set + start time
  int32_t obs_off, n_obs;
  double start_t;
  Poly3HP bbox[6];
};
struct Poly3Dev {
  const Poly3HP *hps;
  const Poly3Seg *segs;
  const Poly3Obs *obs;
  const Poly3World *worlds;
  const int32_t *world_of;                            // (search) world of every query of the launch
  const double *U;                                    // n_u x 3
  int32_t control, n_u;
  double dt, v_max, a_max, j_max, w;
};

// Polyhedron::inside(pt) (decomp_geometry/polyhedron.h): every hyperplane has n.dot(pt - p) <= eps
MPLX_HD bool p3_inside(const Poly3HP *hp, int n_hp, double x, double y, double z) {
  for (int i = 0; i < n_hp; i++) {
    const double dx = x - hp[i].p[0], dy = y - hp[i].p[1], dz = z - hp[i].p[2];
    double s = 0.0;
    s += hp[i].n[0] * dx;
    s += hp[i].n[1] * dy;
    s += hp[i].n[2] * dz;
    if (s > POLY_EPS) return false;
  }
  return true;
}
// Trajectory::evaluate(time).pos / vel / acc / jrk of an obstacle trajectory (mpl_shim trajectory.h)
MPLX_HD void p3_traj_eval(const Poly3Seg *segs, int n_seg, double total_t, double time, double pos[3], double vel[3], double acc[3], double jrk[3]) {
  for (int k = 0; k < 3; k++) pos[k] = vel[k] = acc[k] = jrk[k] = 0.0;
  if (n_seg <= 0) return;
  const double tau = time < 0 ? 0 : (time > total_t ? total_t : time);
  double t0 = 0.0;
  for (int id = 0; id < n_seg; id++) {
    const double t1 = segs[id].T + t0;
    if ((tau >= t0 && tau < t1) || id + 1 == n_seg) {
      const double lt = tau - t0;
      for (int k = 0; k < 3; k++) {
        pos[k] = pp_p(segs[id].c[k], lt);
        vel[k] = pp_v(segs[id].c[k], lt);
        acc[k] = pp_a(segs[id].c[k], lt);
        jrk[k] = pp_j(segs[id].c[k], lt);
      }
      return;
    }
    t0 = t1;
  }
}

// obstacle.inside(pt[, t]) of the three classes (simple_obstacle.h:28, :77-86, :124-135)
MPLX_HD bool p3_inside_static_at(const Poly3Dev &D, const Poly3Obs &o, double x, double y, double z, const double p[3]) {
  return p3_inside(D.hps + o.hp_off, o.n_hp, x - p[0], y - p[1], z - p[2]);
}
MPLX_HD bool p3_inside_linear(const Poly3Dev &D, const Poly3Obs &o, double x, double y, double z, double t) {
  // poly(t): every hyperplane point moves by v t + p + cov_v n t, then Polyhedron::inside
  const Poly3HP *hp = D.hps + o.hp_off;
  const double pt[3] = {x, y, z};
  for (int i = 0; i < o.n_hp; i++) {
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
      const double q = hp[i].p[k] + ((o.v[k] * t + o.p[k]) + (o.cov_v * hp[i].n[k]) * t);
      s += hp[i].n[k] * (pt[k] - q);
    }
    if (s > POLY_EPS) return false;
  }
  return true;
}
MPLX_HD bool p3_inside_nonlinear(const Poly3Dev &D, const Poly3Obs &o, double x, double y, double z, double t) {
  t += o.start_t;
  double wp[3], wv[3], wa[3], wj[3];
  p3_traj_eval(D.segs + o.seg_off, o.n_seg, o.total_t, t, wp, wv, wa, wj);
  const bool there = (t <= o.total_t && t >= 0) || (t < 0 && !o.dis_front) || (t > o.total_t && !o.dis_back);
  return there && p3_inside_static_at(D, o, x, y, z, wp);
}
// PolyMapUtil::isFree(pt, t) restricted to one obstacle (poly_map_util.h:75-88)
MPLX_HD bool p3_point_hits(const Poly3Dev &D, const Poly3Obs &o, double x, double y, double z, double t_rel) {
  return o.kind == 0 ? p3_inside_static_at(D, o, x, y, z, o.p) : o.kind == 1 ? p3_inside_linear(D, o, x, y, z, t_rel) : p3_inside_nonlinear(D, o, x, y, z, t_rel);
}

// collide(pr, PolyhedronObstacle) with the representative point p (primitive_geometry_utils.h:5-39); 1 hit, 0 free, -1 unsupported
template <bool GEN>
MPLX_HD int p3_collide_static_at(const Poly3Dev &D, const double cs[3][6], double T, const Poly3Obs &o, const double p[3]) {
  const Poly3HP *hp = D.hps + o.hp_off;
  for (int h = 0; h < o.n_hp; h++) {
    const double *n = hp[h].n;
    double a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
    for (int i = 0; i < 3; i++) {
      a += n[i] * cs[i][0];
      b += n[i] * cs[i][1];
      c += n[i] * cs[i][2];
      d += n[i] * cs[i][3];
      e += n[i] * cs[i][4];
      f += n[i] * cs[i][5];
    }
    a /= 120.0; b /= 24.0; c /= 6.0; d /= 2.0; e /= 1.0;
    {
      double s = 0.0;
      for (int i = 0; i < 3; i++) s += n[i] * (hp[h].p[i] + p[i]);
      f -= s;
    }
    double ts[GEN ? POLY_MAX_ROOTS : 2];
    const int nr = solve_poly<GEN>(a, b, c, d, e, f, ts);
    if (nr < 0) return -1;
    for (int r = 0; r < nr; r++) {
      const double it = ts[r];
      if (it >= 0 && it <= T && p3_inside_static_at(D, o, pp_p(cs[0], it), pp_p(cs[1], it), pp_p(cs[2], it), p)) return 1;
    }
  }
  return 0;
}
// collide(pr, PolyhedronLinearObstacle, t) (primitive_geometry_utils.h:41-84)
template <bool GEN>
MPLX_HD int p3_collide_linear(const Poly3Dev &D, const double cs[3][6], double T, const Poly3Obs &o, double t) {
  const Poly3HP *hp = D.hps + o.hp_off;
  for (int h = 0; h < o.n_hp; h++) {
    const double *n = hp[h].n;
    const double cov_v[3] = {o.v[0] + o.cov_v * n[0], o.v[1] + o.cov_v * n[1], o.v[2] + o.cov_v * n[2]};
    double a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
    for (int i = 0; i < 3; i++) {
      a += n[i] * cs[i][0];
      b += n[i] * cs[i][1];
      c += n[i] * cs[i][2];
      d += n[i] * cs[i][3];
      e += n[i] * cs[i][4];
      f += n[i] * cs[i][5];
    }
    a /= 120.0; b /= 24.0; c /= 6.0; d /= 2.0;
    {
      double s = 0.0;
      for (int i = 0; i < 3; i++) s += n[i] * cov_v[i];
      e -= s;
      double s2 = 0.0;
      for (int i = 0; i < 3; i++) s2 += n[i] * ((hp[h].p[i] + o.p[i]) + cov_v[i] * t);
      f -= s2;
    }
    double ts[GEN ? POLY_MAX_ROOTS : 2];
    const int nr = solve_poly<GEN>(a, b, c, d, e, f, ts);
    if (nr < 0) return -1;
    for (int r = 0; r < nr; r++) {
      const double it = ts[r];
      if (it >= 0 && it <= T && p3_inside_linear(D, o, pp_p(cs[0], it), pp_p(cs[1], it), pp_p(cs[2], it), it + t)) return 1;
    }
  }
  return 0;
}
// collide(pr, PolyhedronNonlinearObstacle, t) (primitive_geometry_utils.h:86-173)
template <bool GEN>
MPLX_HD int p3_collide_nonlinear(const Poly3Dev &D, const double cs[3][6], double prT, const Poly3Obs &o, double t) {
  const Poly3Seg *segs = D.segs + o.seg_off;
  const double traj_t = t + o.start_t;
  int start_id = -1;
  double T = 0.0;  // current segment start time
  for (int i = 0; i < o.n_seg; i++) {
    if (traj_t >= T && traj_t < T + segs[i].T) {
      start_id = i;
      break;
    }
    T += segs[i].T;
  }
  if (start_id < 0) {  // outside the trajectory's time span: its clamped end state as a static obstacle, or nothing
    double wp[3], wv[3], wa[3], wj[3];
    p3_traj_eval(segs, o.n_seg, o.total_t, traj_t, wp, wv, wa, wj);
    const bool there = (traj_t <= o.total_t && traj_t >= 0) || (traj_t < 0 && !o.dis_front) || (traj_t > o.total_t && !o.dis_back);
    return there ? p3_collide_static_at<GEN>(D, cs, prT, o, wp) : 0;
  }
  const Poly3HP *hp = D.hps + o.hp_off;
  for (int id = start_id; id < o.n_seg; id++) {
    const double t_residual = T - traj_t < 0 ? 0 : T - traj_t;
    const double start_t = t_residual <= 0 ? traj_t : T;
    if (t_residual > prT) break;
    double wp[3], wv[3], wa[3], wj[3];
    p3_traj_eval(segs, o.n_seg, o.total_t, start_t, wp, wv, wa, wj);
    for (int h = 0; h < o.n_hp; h++) {
      const double *n = hp[h].n;
      double a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
      for (int i = 0; i < 3; i++) {
        a += n[i] * cs[i][0];
        b += n[i] * cs[i][1];
        c += n[i] * cs[i][2] - n[i] * wj[i];
        d += n[i] * cs[i][3] - n[i] * wa[i];
        e += n[i] * cs[i][4] - n[i] * wv[i];
        f += n[i] * cs[i][5] - n[i] * (hp[h].p[i] + wp[i]);
      }
      a /= 120; b /= 24; c /= 6; d /= 2;
      double ts[GEN ? POLY_MAX_ROOTS : 2];
      const int nr = solve_poly<GEN>(a, b, c, d, e, f, ts);
      if (nr < 0) return -1;
      for (int r = 0; r < nr; r++) {
        const double it = ts[r];
        if (it >= t_residual && it <= prT && T + segs[id].T >= it + start_t && T <= it + start_t &&
            p3_inside_nonlinear(D, o, pp_p(cs[0], it), pp_p(cs[1], it), pp_p(cs[2], it), it + t))
          return 1;
      }
    }
    T += segs[id].T;
  }
  return 0;
}
// PolyMapUtil::isFree(pr, t) restricted to one obstacle (poly_map_util.h:92-109; the start-point test is separate)
template <bool GEN>
MPLX_HD int p3_prim_hits(const Poly3Dev &D, const double cs[3][6], double T, const Poly3Obs &o, double t_rel) {
  return o.kind == 0 ? p3_collide_static_at<GEN>(D, cs, T, o, o.p) : o.kind == 1 ? p3_collide_linear<GEN>(D, cs, T, o, t_rel) : p3_collide_nonlinear<GEN>(D, cs, T, o, t_rel);
}

// Primitive<3>(curr, u, dt) coefficients (mpl_shim primitive.h)
MPLX_HD void p3_prim_build(int control, const double pos[3], const double vel[3], const double acc[3], const double jrk[3], const double u[3], double cs[3][6]) {
  const int kind = control & 15;
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 6; k++) cs[i][k] = 0.0;
    if (kind == CTRL_VEL) { cs[i][4] = u[i]; cs[i][5] = pos[i]; }
    else if (kind == CTRL_ACC) { cs[i][3] = u[i]; cs[i][4] = vel[i]; cs[i][5] = pos[i]; }
    else if (kind == CTRL_JRK) { cs[i][2] = u[i]; cs[i][3] = acc[i]; cs[i][4] = vel[i]; cs[i][5] = pos[i]; }
    else { cs[i][1] = u[i]; cs[i][2] = jrk[i]; cs[i][3] = acc[i]; cs[i][4] = vel[i]; cs[i][5] = pos[i]; }
  }
}
// validate_primitive (mpl_shim primitive.h): ACC / JRK / SNP check max |vel| per axis, JRK / SNP max |acc|, SNP max |jrk|
MPLX_HD bool p3_validate(int control, const double cs[3][6], double T, double v_max, double a_max, double j_max) {
  const int kind = control & 15;
  if (kind == CTRL_ACC || kind == CTRL_JRK || kind == CTRL_SNP)
    for (int i = 0; i < 3; i++)
      if (v_max > 0 && poly_max_abs(cs[i], 1, T) > v_max) return false;
  if (kind == CTRL_JRK || kind == CTRL_SNP)
    for (int i = 0; i < 3; i++)
      if (a_max > 0 && poly_max_abs(cs[i], 2, T) > a_max) return false;
  if (kind == CTRL_SNP)
    for (int i = 0; i < 3; i++)
      if (j_max > 0 && poly_max_abs(cs[i], 3, T) > j_max) return false;
  return true;
}
// env_poly_map::calculate_intrinsic_cost: pr.J(pr.control()) + 0.001 * pr.J(Control::VEL) + w dt (env_poly_map.h:71-73)
MPLX_HD double p3_intrinsic_cost(int control, const double cs[3][6], double T, double w, double dt) {
  double jc = 0;
  for (int k = 0; k < 3; k++) jc += pp_J(cs[k], T, control);
  double jv = 0;
  for (int k = 0; k < 3; k++) jv += pp_J(cs[k], T, CTRL_VEL);
  return jc + 0.001 * jv + w * dt;
}

#ifdef __HIPCC__
// isFree(start.pos, t) over the obstacles of world W, then -- unless that failed -- isFree(pr, t) of every valid primitive
// (cs[i], i < n_u) against every obstacle, one (primitive, obstacle) pair per lane.  ORs into hit[i], sets *start_hit and
// *unsupported.  Every thread of the workgroup must call.
template <int BLOCK, bool GEN>
__device__ __forceinline__ void p3_collide_all(const Poly3Dev &D, const Poly3World &W, const double (*cs)[3][6], const int32_t *valid, int n_u, double T, double t_rel,
                                               int32_t *hit, int32_t *unsupported, int32_t *start_hit, int tid) {
  const int n_obs = W.n_obs;
  const Poly3Obs *obs = D.obs + W.obs_off;
  // pr.evaluate(0).pos: the node position, whatever the primitive
  const double x0 = pp_p(cs[0][0], 0.0), y0 = pp_p(cs[0][1], 0.0), z0 = pp_p(cs[0][2], 0.0);
  for (int j = tid; j < n_obs; j += BLOCK)
    if (p3_point_hits(D, obs[j], x0, y0, z0, t_rel)) *start_hit = 1;
  __syncthreads();
  if (*start_hit) return;  // (uniform: every primitive is blocked)
  const int pairs = n_u * n_obs;
  for (int e = tid; e < pairs; e += BLOCK) {
    const int i = e / n_obs, j = e - (e / n_obs) * n_obs;
    if (!valid[i]) continue;
    double c[3][6];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 6; b++) c[a][b] = cs[i][a][b];
    const int r = p3_prim_hits<GEN>(D, c, T, obs[j], t_rel);
    if (r < 0) *unsupported = 1;
    if (r > 0) hit[i] = 1;
  }
  __syncthreads();
}

// One successor of env_poly_map<3>::get_succ (mirrors mplx_poly3_succ)
struct Poly3SuccOut {
  double state[13];  // pos3 vel3 acc3 jrk3 t
  double cost;       // intrinsic cost, or +inf when PolyMapUtil::isFree(pr, t) fails
  int32_t action, valid;
};

// env_poly_map<3>::get_succ for K states (pos3 vel3 acc3 jrk3 t): one workgroup per state.
template <int BLOCK, bool GEN>
__global__ __launch_bounds__(BLOCK) void poly3_get_succ_kernel(Poly3Dev D, int K, const int32_t *world_of, const double *states, Poly3SuccOut *out, int32_t *flags) {
  __shared__ double cs[POLY3_MAX_U][3][6];
  __shared__ int32_t valid[POLY3_MAX_U], hit[POLY3_MAX_U];
  __shared__ int32_t start_hit, unsupported;
  const int tid = threadIdx.x;
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    const double *st = states + 13 * (size_t)k;
    const Poly3World &W = D.worlds[world_of[k]];
    const double T = D.dt, t_rel = st[12] - W.start_t;
    if (tid == 0) { start_hit = 0; unsupported = 0; }
    if (tid < D.n_u) {
      double c[3][6];
      p3_prim_build(D.control, st, st + 3, st + 6, st + 9, D.U + 3 * tid, c);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 6; j++) cs[tid][i][j] = c[i][j];
      valid[tid] = (p3_inside(W.bbox, 6, pp_p(c[0], T), pp_p(c[1], T), pp_p(c[2], T)) && p3_validate(D.control, c, T, D.v_max, D.a_max, D.j_max)) ? 1 : 0;
      hit[tid] = 0;
    }
    __syncthreads();
    p3_collide_all<BLOCK, GEN>(D, W, cs, valid, D.n_u, T, t_rel, hit, &unsupported, &start_hit, tid);
    if (tid < D.n_u) {
      Poly3SuccOut &o = out[(size_t)k * D.n_u + tid];
      double c[3][6];
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 6; b++) c[a][b] = cs[tid][a][b];
      for (int ax = 0; ax < 3; ax++) {
        o.state[ax] = pp_p(c[ax], T);
        o.state[3 + ax] = pp_v(c[ax], T);
        o.state[6 + ax] = pp_a(c[ax], T);
        o.state[9 + ax] = pp_j(c[ax], T);
      }
      o.state[12] = st[12] + D.dt;
      o.action = tid;
      o.valid = valid[tid];
      o.cost = (start_hit || hit[tid]) ? INFINITY : p3_intrinsic_cost(D.control, c, T, D.w, D.dt);
    }
    if (tid == 0 && unsupported) atomicOr(flags, 1);
    __syncthreads();
  }
}

// ---- GraphSearch::Astar over env_poly_map<3>: the per-query steps of mplx_search_steps.h around the 3-D get_succ.
// Time-keyed states (key: the state's integers + round(t / 0.1), env_poly_map.h:63-64), the edge cost travels with the lane
// and recoverTraj recomputes it from the parent state; PlannerBase::plan's start test is isInside(start.pos).
template <int BLOCK, int CONTROL, bool GEN>
__global__ __launch_bounds__(BLOCK) void astar_poly3_kernel(SearchParams P, Poly3Dev D) {
  static_assert(CONTROL == CTRL_ACC || CONTROL == CTRL_JRK, "time-keyed states: the key of an SNP state would need 13 integers");
  constexpr int ns = key_len_c(CONTROL), NK = ns + 1;
  __shared__ Smem<BLOCK> S;
  __shared__ double pcs[POLY3_MAX_U][3][6];
  __shared__ int32_t pvalid[POLY3_MAX_U], phit[POLY3_MAX_U];
  __shared__ int32_t pstart_hit, punsupported;
  __shared__ double pU[POLY3_MAX_U][3];
  using V = QView<BLOCK, CONTROL>;
  const int tid = threadIdx.x;
  const V Q{P, S, P.bkt_head + (size_t)blockIdx.x * 2 * NB * NSUB};
  for (int i = tid; i < 3 * P.n_u; i += BLOCK) pU[i / 3][i % 3] = D.U[i];
  for (;;) {
    if (tid == 0) {
      S.q_index = atomicAdd(P.next_query, 1);
      if (guard_abort(P)) S.q_index = P.nq;  // the host has given up on this launch: take no further query
    }
    __syncthreads();
    const int qi = S.q_index;
    if (qi >= P.nq) break;
    const int q = P.order[qi];
    const QueryIn &in = P.queries[q];
    const Poly3World &W = D.worlds[D.world_of[q]];
    const unsigned long long t_begin = wall_clock64();
    query_reset(Q, in, (uint32_t)P.n_u, tid);
    if (tid == 0) {
      punsupported = 0;
      // ENV_->is_free(start.pos): inside the bounding box
      query_admit(Q, in, p3_inside(W.bbox, 6, in.start.p[0], in.start.p[1], in.start.p[2]), is_goal_state(in.start, in.goal, in.goal_control, P.tol_pos, P.tol_vel, P.tol_acc));
    }
    __syncthreads();
    uint32_t goal_id = NIL;
    if (S.status < 0) {
      // (the start's key carries the start time)
      const bool started = query_start<NK, 0>(Q, in, q, tid, (int32_t)round(in.start_t / 0.1), 0.0, [&](const int32_t *key) { return get_heur(S.hp, CONTROL, in.start, key, NK); });
      if (started) for (;;) {
        while (S.n_near + S.reserve > (uint32_t)NC) {
          evict_half(Q, tid);
          __syncthreads();
        }
        const bool popped = pop_min<BLOCK, CONTROL, Smem<BLOCK>, NK>(Q, tid);
        if (!popped) {
          if (tid == 0) S.status = 1;
          __syncthreads();
          break;
        }
        const uint32_t cur = S.cur_id;
        if (tid == 0) {
          S.c_expanded++;
          S.c_closed++;
          S.c_hash = S.c_hash * 0x100000001B3ull + (unsigned long long)(cur + 1u);
          if (P.rec_ids && S.c_expanded <= P.cap_rec) P.rec_ids[(size_t)q * P.cap_rec + (S.c_expanded - 1)] = (int32_t)cur;
          S.flag = 0;
          pstart_hit = 0;
        }
        // ---- env_poly_map<3>::get_succ(curr): S.cur[0] = pos3 vel3 acc3 jrk3, S.cur[0][12] = curr.t
        const double T = P.dt, cur_t = S.cur[0][12], t_rel = cur_t - W.start_t;
        LaneSucc L;
        L.valid = false; L.blocked = false; L.reads = 0;
        double lane_cost = 0.0;
        if (tid < P.n_u) {
          const double zero3[3] = {0.0, 0.0, 0.0};
          double c[3][6];
          p3_prim_build(CONTROL, &S.cur[0][0], &S.cur[0][3], CONTROL == CTRL_JRK ? &S.cur[0][6] : zero3, zero3, pU[tid], c);
          for (int i = 0; i < 3; i++)
            for (int j = 0; j < 6; j++) pcs[tid][i][j] = c[i][j];
          for (int k = 0; k < 3; k++) {
            L.tn.p[k] = pp_p(c[k], T);
            L.tn.v[k] = pp_v(c[k], T);
            L.tn.a[k] = CONTROL == CTRL_JRK ? pp_a(c[k], T) : 0.0;
            L.tn.j[k] = 0.0;
          }
          pvalid[tid] = (p3_inside(W.bbox, 6, L.tn.p[0], L.tn.p[1], L.tn.p[2]) && p3_validate(CONTROL, c, T, P.v_max, P.a_max, P.j_max)) ? 1 : 0;
          phit[tid] = 0;
          lane_cost = p3_intrinsic_cost(CONTROL, c, T, P.w, P.dt);
          state_key_c<CONTROL>(L.tn, L.key);
          L.key[ns] = (int32_t)round((cur_t + P.dt) / 0.1);
        }
        __syncthreads();
        // isFree(start.pos, t) and isFree(pr, t) of all primitives against all obstacles
        p3_collide_all<BLOCK, GEN>(D, W, pcs, pvalid, P.n_u, T, t_rel, phit, &punsupported, &pstart_hit, tid);
        if (tid < P.n_u) {
          L.valid = pvalid[tid] != 0;
          L.blocked = L.valid && (pstart_hit || phit[tid]);
        }
        const bool act = L.valid && !L.blocked;
        {
          uint32_t tot;
          block_excl_scan<BLOCK>((L.valid ? 1u : 0u) | (act ? 1u << 10 : 0u), S, tid, tot);
          if (tid == 0) {
            S.c_prims += (unsigned long long)P.n_u;
            S.c_succ += tot & 0x3FFu;
            S.c_succ_finite += tot >> 10;
            if (punsupported) S.status = 5;
          }
        }
        const unsigned long long h64 = act ? key_hash64(L.key, NK) : 0ull;
        dup_probe<BLOCK>(S, act, h64, tid);  // (its first barrier publishes the status)
        if (S.status >= 0) break;
        if (!S.flag) {
          commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, NK, false>(Q, tid, q, act, L, h64, lane_cost, (uint32_t)tid);
        } else {
          for (int i = 0; i < P.n_u && S.status < 0; i++)
            commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, NK, false>(Q, tid, q, act && tid == i, L, h64, lane_cost, (uint32_t)tid);
        }
        __syncthreads();
        if (S.status >= 0) break;  // pool full
        if (search_ended(Q, q, tid, [&](const State &s) { return is_goal_state(s, S.hp.goal, S.hp.goal_control, P.tol_pos, P.tol_vel, P.tol_acc); })) break;
      }
      goal_id = S.cur_id;
      clear_buckets(Q, tid);
    }
    __syncthreads();
    if (tid == 0)  // recoverTraj + results
      query_report<0>(Q, q, goal_id, [&](uint32_t parent, uint32_t action) {  // calculate_intrinsic_cost of Primitive(parent, U[action], dt)
        const double *st = V::state(Q.node(parent));
        const double zero3[3] = {0.0, 0.0, 0.0};
        double c[3][6];
        p3_prim_build(CONTROL, st, st + 3, CONTROL == CTRL_JRK ? st + 6 : zero3, zero3, D.U + 3 * (action & EDGE_ACTION_MASK), c);
        return p3_intrinsic_cost(CONTROL, c, P.dt, P.w, P.dt);
      }, SpecCounts{}, t_begin);
    publish_chunk_tables(Q, q, tid);
    __syncthreads();
  }
}
#endif

}  // namespace mplx
