/**
 * @file poly3_device.h  (mplx shim: the device plumbing of PolyMapPlanner<3>)
 *
 * What MPL::PolyMapPlanner<3>::plan() (poly_map_planner.h of this shim) does on the device, with no reference header in
 * sight: the planner's set-up and its one world packed into the arrays of include/mplx.h's mplx_poly3_* calls, the plan
 * with the pool-doubling retry, and the read-back of the trajectory (actions, node ids, states), of the state space
 * (getCloseSet / getOpenSet) and of the expansion order (getExpandedNodes).  The predecessor records behind
 * getValidPrimitives / getAllPrimitives are fetched lazily (poly3_space_fetch: mplx_poly3_result_space / _edges / _blocked),
 * keyed on mplx_poly3_plan_epoch by the rule of poly2_space.h: the device object serves every 3-D planner of the process, so
 * when another planner has planned there since, the space is gone -- a red refusal, nothing fetched.  A program that does not
 * have the reference's headers -- a test driver -- plans through this header exactly as the shim's planner does.
 */
#ifndef MPLX_SHIM_POLY3_DEVICE_H
#define MPLX_SHIM_POLY3_DEVICE_H

#include <mplx.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mplx_shim {

/// one obstacle of a 3-D world: kind 0 static, 1 linear, 2 nonlinear; hp: n x {px, py, pz, nx, ny, nz}; segs: n x {cx[6], cy[6], cz[6], T}
struct Poly3Obstacle {
  int kind = 0;
  std::vector<double> hp;
  double p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, cov_v = 0;
  std::vector<double> segs;
  double start_t = 0;
  bool dis_front = false, dis_back = false;
};
/// one PlannerBase::plan call of a 3-D planner: set-up, world, start / goal (13 doubles: pos3 vel3 acc3 jrk3 t)
struct Poly3Query {
  int control = MPLX_ACC;
  std::vector<double> U;  // n_u x 3
  double dt = 1, v_max = -1, a_max = -1, j_max = -1, w = 10;
  double ori[3] = {0, 0, 0}, dim[3] = {0, 0, 0}, start_t = 0;
  std::vector<Poly3Obstacle> obstacles;
  double start[13] = {0}, goal[13] = {0};
  double eps = 1, tol_pos = 0.5, tol_vel = -1;
  int max_num = -1, heur_ignore_dynamics = 0;
};
/// what the plan leaves: the result, the trajectory start -> goal (actions, node ids, states (len + 1) x 13), the state space
/// (positions, closed / opened flags, in id order) and the expansion order (node ids)
struct Poly3Plan {
  mplx_result res = mplx_result();
  std::vector<int32_t> actions, node_ids, expanded;
  std::vector<double> states, node_pos;
  std::vector<int32_t> closed, opened;
  uint64_t epoch = 0;  // mplx_poly3_plan_epoch of the shared device object right after this plan (0: no plan ran on the device)
};
/// the predecessor records of one 3-D plan on the host: states n x 13 (pos3 vel3 acc3 jrk3 t) in id order, the records with
/// finite cost (child, parent, action) in push_back order and the blocked ones (parent, action), parents in id order
struct Poly3Space {
  bool fetched = false;          // states and valid records are here
  bool blocked_fetched = false;  // the blocked records too
  std::vector<double> states;
  std::vector<int32_t> child, parent, action;
  std::vector<int32_t> blocked_parent, blocked_action;
  size_t n_nodes() const { return states.size() / 13; }
};

/// One device object serves every 3-D planner of the process (the reference constructs a new planner per plan: robot.hpp:109)
inline mplx_poly3 *poly3_shared_device(bool destroy = false) {
  static mplx_poly3 *p = nullptr;
  if (destroy) { if (p) mplx_poly3_destroy(p); p = nullptr; return nullptr; }
  if (!p && mplx_poly3_create(0, &p) != MPLX_OK) {
    printf("\x1b[31m[PolyMapPlanner] %s\n\x1b[0m", mplx_poly3_last_error(nullptr));
    p = nullptr;
  }
  return p;
}
/// pool capacities of that object (states, predecessor records, OPEN-log entries); doubled on MPLX_PLAN_POOL_FULL
inline uint64_t *poly3_shared_capacity() {
  static uint64_t cap[3] = {1u << 20, 1u << 22, 1u << 21};
  return cap;
}
inline bool poly3_check(mplx_poly3 *p, int rc) {
  if (rc == MPLX_OK) return true;
  printf("\x1b[31m[PolyMapPlanner] %s\n\x1b[0m", mplx_poly3_last_error(p));
  return false;
}
/// uploads the query's set-up and world (world 0), plans -- doubling the pools on MPLX_PLAN_POOL_FULL, at most six times --
/// and reads back what the planner's getters answer.  false: a device call failed (the message is printed); otherwise
/// out.res.status says how the search ended.
inline bool poly3_plan(const Poly3Query &q, Poly3Plan &out) {
  out = Poly3Plan();
  mplx_poly3 *p = poly3_shared_device();
  if (!p) return false;
  const int32_t n_u = (int32_t)(q.U.size() / 3);
  if (!poly3_check(p, mplx_poly3_config(p, q.control, n_u, q.U.data(), q.dt, q.v_max, q.a_max, q.j_max, q.w))) return false;
  if (!poly3_check(p, mplx_poly3_begin(p, 1))) return false;
  if (!poly3_check(p, mplx_poly3_set_world(p, 0, q.ori, q.dim, q.start_t))) return false;
  for (const Poly3Obstacle &o : q.obstacles) {
    const int32_t n_hp = (int32_t)(o.hp.size() / 6);
    int rc = MPLX_ERR_ARG;
    if (o.kind == 0) rc = mplx_poly3_add_static(p, 0, n_hp, o.hp.data(), o.p);
    else if (o.kind == 1) rc = mplx_poly3_add_linear(p, 0, n_hp, o.hp.data(), o.p, o.v, o.cov_v);
    else rc = mplx_poly3_add_nonlinear(p, 0, n_hp, o.hp.data(), (int32_t)(o.segs.size() / 19), o.segs.data(), o.start_t, o.dis_front ? 1 : 0, o.dis_back ? 1 : 0);
    if (!poly3_check(p, rc)) return false;
  }
  if (!poly3_check(p, mplx_poly3_commit(p))) return false;
  const uint32_t rec = 1u << 20;  // (expansion order of the first 2^20 expansions: getExpandedNodes)
  if (!poly3_check(p, mplx_poly3_set_record(p, rec))) return false;
  uint64_t *cap = poly3_shared_capacity();
  const int32_t world = 0;
  for (int attempt = 0;; attempt++) {
    if (!poly3_check(p, mplx_poly3_set_capacity(p, 1, cap[0], cap[1], cap[2]))) return false;
    if (!poly3_check(p, mplx_poly3_plan_batch(p, 1, &world, q.start, q.goal, q.eps, q.tol_pos, q.tol_vel, q.max_num, q.heur_ignore_dynamics, &out.res)))
      return false;
    if (out.res.status != MPLX_PLAN_POOL_FULL || attempt >= 6) break;
    for (int k = 0; k < 3; k++) cap[k] *= 2;  // (the reference grows std containers: grow the device pools and search again)
    printf("\x1b[36m[PolyMapPlanner] device pools exhausted: doubled, planning again\n\x1b[0m");
  }
  const int len = out.res.status == MPLX_PLAN_OK ? out.res.traj_len : 0;
  if (len > 0) {
    out.actions.resize((size_t)len);
    out.node_ids.resize((size_t)len + 1);
    out.states.resize((size_t)(len + 1) * 13);
    if (!poly3_check(p, mplx_poly3_result_traj(p, 0, out.actions.data(), out.node_ids.data(), out.states.data()))) return false;
  }
  const uint64_t n = out.res.n_nodes;
  if (n > 0) {
    std::vector<mplx_waypoint> wps((size_t)n);
    out.closed.resize((size_t)n);
    out.opened.resize((size_t)n);
    if (!poly3_check(p, mplx_poly3_result_nodes(p, 0, n, wps.data(), nullptr, out.closed.data(), out.opened.data()))) return false;
    out.node_pos.resize((size_t)n * 3);
    for (size_t i = 0; i < (size_t)n; i++)
      for (int k = 0; k < 3; k++) out.node_pos[3 * i + (size_t)k] = wps[i].pos[k];
  }
  out.epoch = mplx_poly3_plan_epoch(p);  // (the lazy getters answer while this is still the device object's last plan)
  if (out.res.n_expanded > 0) {
    uint32_t ne = 0;
    out.expanded.resize((size_t)(out.res.n_expanded < rec ? out.res.n_expanded : rec));
    if (!poly3_check(p, mplx_poly3_result_expanded(p, 0, (uint32_t)out.expanded.size(), out.expanded.data(), &ne))) return false;
    out.expanded.resize(ne);
  }
  return true;
}

inline void poly3_refuse(const char *what, const char *why) { printf("\x1b[31m[PolyMapPlanner] %s refused: %s\n\x1b[0m", what, why); }
/// Query 0 of the plan the caller noted `epoch` after (Poly3Plan::epoch).  with_blocked: the blocked records too (re-derived on
/// the device when first asked for).  false: refused or a device call failed (the message is printed), `out` is left empty.
/// A planner that has not planned on the device is refused without touching the device.
inline bool poly3_space_fetch(uint64_t epoch, const mplx_result &res, bool with_blocked, Poly3Space &out, const char *what) {
  if (epoch == 0) {
    poly3_refuse(what, "this PolyMapPlanner3D has not planned on the device");
    out = Poly3Space();
    return false;
  }
  mplx_poly3 *p = poly3_shared_device();
  if (!p || mplx_poly3_plan_epoch(p) != epoch) {
    poly3_refuse(what, "another planner has planned on the shared device object since this planner's plan(): its state space is gone");
    out = Poly3Space();
    return false;
  }
  if (!out.fetched) {
    out = Poly3Space();
    const uint64_t n = res.n_nodes;
    if (n > 0) {
      out.states.resize((size_t)n * 13);
      if (!poly3_check(p, mplx_poly3_result_space(p, 0, n, out.states.data(), nullptr, nullptr, nullptr, nullptr))) { out = Poly3Space(); return false; }
      uint64_t ne = 0;
      if (!poly3_check(p, mplx_poly3_result_edges(p, 0, 0, nullptr, nullptr, nullptr, &ne))) { out = Poly3Space(); return false; }
      out.child.resize((size_t)ne); out.parent.resize((size_t)ne); out.action.resize((size_t)ne);
      if (ne && !poly3_check(p, mplx_poly3_result_edges(p, 0, ne, out.child.data(), out.parent.data(), out.action.data(), &ne))) { out = Poly3Space(); return false; }
    }
    out.fetched = true;
  }
  if (with_blocked && !out.blocked_fetched) {
    uint64_t nb = 0;
    if (!poly3_check(p, mplx_poly3_result_blocked(p, 0, 0, nullptr, nullptr, &nb))) return false;
    out.blocked_parent.resize((size_t)nb); out.blocked_action.resize((size_t)nb);
    if (nb && !poly3_check(p, mplx_poly3_result_blocked(p, 0, nb, out.blocked_parent.data(), out.blocked_action.data(), &nb))) {
      out.blocked_parent.clear(); out.blocked_action.clear();
      return false;
    }
    out.blocked_fetched = true;
  }
  return true;
}

}  // namespace mplx_shim
#endif
