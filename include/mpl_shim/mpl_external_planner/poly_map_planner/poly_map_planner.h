/**
 * @file poly_map_planner.h  (mplx shim of <mpl_external_planner/poly_map_planner/poly_map_planner.h>)
 *
 * MPL::PolyMapPlanner<Dim> with the search done on the GPU (libmplx.so: mplx_poly_*).  Put include/mpl_shim AHEAD of the
 * reference's mpl_external_planner/include on the include path: this file then replaces the reference's 53-line planner
 * glue of the same name, and everything else of that directory -- env_poly_map.h, poly_map_util.h,
 * primitive_geometry_utils.h, simple_obstacle.h -- is still the reference's own, unchanged (it is included below from
 * where it lies).  Class name, method names and argument meaning are the reference's (poly_map_planner.h:17-93), so its
 * callers -- mpl_test_node/src/robot.hpp:92-133 (planner_ptr.reset(new MPL::PolyMapPlanner<Dim>(false)) ... plan(start_,
 * goal_)), robot_team.hpp, poly_map_planner_node.cpp -- compile and run unchanged.
 *
 * Why a replacement and not a hook: the reference's planner searches through ENV_, a host C++ object whose get_succ is a
 * virtual call per expansion; a device search cannot call it, and PolyMapUtil keeps its obstacles private.  Here the
 * setters keep a copy of the obstacles next to handing them to the reference's PolyMapUtil (which still answers
 * getPolyhedrons / getBoundingBox / getLinearObstacles and is what ENV_ wraps), and plan() uploads them as ONE world of
 * an mplx_poly object and runs PlannerBase::plan there (time-keyed states, env_poly_map.h:63-64; cost
 * J + 0.001 J(VEL) + w dt, :71-73).  2-D like every in-tree caller (multi_robot_node.cpp, poly_map_planner_node.cpp); a
 * PolyMapPlanner3D (poly_map_planner.h:107, robot.hpp:229) plans through mplx_poly3_* instead, by way of the reference-free
 * plumbing of poly3_device.h, and serves all five getters from the device too -- getValidPrimitives / getAllPrimitives lazily,
 * through mplx_poly3_result_space / _edges / _blocked (3-D LPA* is refused).
 * A 2-D planner serves getCloseSet / getOpenSet / getExpandedNodes / getValidPrimitives / getAllPrimitives from the device as
 * well (poly_map_planner_node.cpp:105-124, poly_map_replanner_node.cpp:156-158,184,234), through the reference-free
 * poly2_space.h: lazily from the shared device object in A* mode, from its own LPA* handle with setLPAstar(true).
 * With setLPAstar(true) (poly_map_replanner_node.cpp:352) the planner keeps a device-resident LPA* state space of its own
 * (mplx_plpa_*): updateNodes() (:61-93) re-tests every stored predecessor primitive against the obstacles as they are now and
 * fills getBlockedPrimitives / getClearedPrimitives, plan() repairs, getSubStateSpace(k) re-roots (round 6).
 */
#ifndef MPLX_SHIM_POLY_MAP_PLANNER_H
#define MPLX_SHIM_POLY_MAP_PLANNER_H

#include <mpl_external_planner/poly_map_planner/env_poly_map.h>  // the reference's own (next on the include path)
#include <mpl_planner/common/planner_base.h>
#include <mplx.h>

#include "poly2_space.h"
#include "poly3_device.h"

#include <vector>

namespace MPL {

/// One device object serves every planner of the process: the reference's robots construct a NEW PolyMapPlanner for
/// every plan() (robot.hpp:109), and device pools are not something to allocate at 2 Hz per robot.
inline mplx_poly *shared_poly_device(bool destroy = false) {
  static mplx_poly *p = nullptr;
  if (destroy) { if (p) mplx_poly_destroy(p); p = nullptr; return nullptr; }
  if (!p) {
    if (mplx_poly_create(0, &p) != MPLX_OK) {
      printf(ANSI_COLOR_RED "[PolyMapPlanner] %s\n" ANSI_COLOR_RESET, mplx_poly_last_error(nullptr));
      p = nullptr;
    }
  }
  return p;
}
/// pool capacities of that object (states, predecessor records, OPEN-log entries of one search); doubled on MPLX_PLAN_POOL_FULL
inline uint64_t *shared_poly_capacity() {
  static uint64_t cap[3] = {1u << 20, 1u << 22, 1u << 21};
  return cap;
}

template <int Dim>
class PolyMapPlanner : public PlannerBase<Dim, Waypoint<Dim>> {
  typedef PlannerBase<Dim, Waypoint<Dim>> Base;

 public:
  PolyMapPlanner(bool verbose = false) {
    this->planner_verbose_ = verbose;
    if (this->planner_verbose_) printf(ANSI_COLOR_CYAN "[PolyMapPlanner] PLANNER VERBOSE ON (mplx back-end)\n" ANSI_COLOR_RESET);
  }
  /// Set map util (poly_map_planner.h:30-34)
  void setMap(const Vecf<Dim> &ori, const Vecf<Dim> &dim) {
    map_util_.reset(new PolyMapUtil<Dim>());
    map_util_->setBoundingBox(ori, dim);
    this->ENV_.reset(new MPL::env_poly_map<Dim>(map_util_));
    this->apply_to_env();  // (the reference's setters forward to ENV_, which exists only from here on)
    ori_ = ori;
    dim_ = dim;
    has_map_ = true;
  }
  void setStartTime(decimal_t t) { map_util_->setStartTime(t); start_t_ = t; }
  void setStaticObstacles(const vec_E<PolyhedronObstacle<Dim>> &obs) { map_util_->setStaticObstacle(obs); static_obs_ = obs; }
  void setLinearObstacles(const vec_E<PolyhedronLinearObstacle<Dim>> &obs) { map_util_->setLinearObstacle(obs); linear_obs_ = obs; }
  void setNonlinearObstacles(const vec_E<PolyhedronNonlinearObstacle<Dim>> &obs) { map_util_->setNonlinearObstacle(obs); nonlinear_obs_ = obs; }
  vec_E<Polyhedron<Dim>> getPolyhedrons(decimal_t time) const { return map_util_->getPolyhedrons(time); }
  vec_E<PolyhedronLinearObstacle<Dim>> getLinearObstacles() const { return map_util_->getLinearObstacles(); }
  Polyhedron<Dim> getBoundingBox() const { return map_util_->getBoundingBox(); }

  ~PolyMapPlanner() {
    if (lpa_) mplx_plpa_destroy(lpa_);
  }
  /// poly_map_planner.h:61-93: after setLinearObstacles / setStartTime, re-test every stored predecessor primitive of the kept LPA*
  /// state space (forward_action + isFree(pr, pred.t)); what became blocked / free is collected, costs change, look-ahead values follow
  void updateNodes() {
    blocked_prs_.clear();
    cleared_prs_.clear();
    if (Dim == 3) { refuse3("updateNodes()"); return; }
    if (!lpa_ || !mplx_plpa_initialized(lpa_)) return;  // (if (!this->ss_ptr_) return;)
    space_ = mplx_shim::Poly2Space();
    mplx_poly *p = shared_poly_device();
    if (!p || !upload(p, lpa_control_)) return;
    uint64_t nb = 0, nc = 0, n = 0;
    if (!lcheck(mplx_plpa_update_nodes(lpa_, 0, &nb, &nc))) return;
    if (!lcheck(mplx_plpa_changed(lpa_, 0, nullptr, nullptr, &n)) || n == 0) return;
    // parent state, action and now-blocked bit of the changed entries, gathered on the device in the order of mplx_plpa_changed:
    // O(changed) over the bus, where two dumps of the whole space used to be decoded here
    std::vector<double> states((size_t)n * 9);
    std::vector<int32_t> action((size_t)n), now((size_t)n);
    if (!lcheck(mplx_plpa_export_changed(lpa_, n, states.data(), action.data(), now.data(), &n))) return;
    if (n > (uint64_t)action.size()) n = action.size();
    for (size_t i = 0; i < (size_t)n; i++) {  // the primitive of a changed entry: forward_action(pred_coord, pred_action_id)
      const double *st = &states[i * 9];
      Waypoint<Dim> w((Control::Control)lpa_control_);
      for (int k = 0; k < 2; k++) { w.pos(k) = st[k]; w.vel(k) = st[2 + k]; w.acc(k) = st[4 + k]; w.jrk(k) = st[6 + k]; }
      w.t = st[8];
      const Primitive<Dim> pr(w, this->U_vec_[(size_t)action[i]], this->dt_);
      (now[i] ? blocked_prs_ : cleared_prs_).push_back(pr);
    }
  }
  /// PlannerBase::initialized() / getSubStateSpace(time_step) of the LPA* planner (poly_map_replanner_node.cpp:231)
  bool initialized() { return lpa_ && mplx_plpa_initialized(lpa_); }
  void getSubStateSpace(int time_step) {
    if (Dim == 3) { refuse3("getSubStateSpace()"); return; }
    if (!lpa_ || !mplx_plpa_initialized(lpa_)) return;
    space_ = mplx_shim::Poly2Space();
    mplx_poly *p = shared_poly_device();
    if (!p || !upload(p, lpa_control_)) return;
    lcheck(mplx_plpa_sub_state_space(lpa_, 0, time_step));
  }
  vec_E<Primitive<Dim>> getBlockedPrimitives() { return blocked_prs_; }
  vec_E<Primitive<Dim>> getClearedPrimitives() { return cleared_prs_; }

  /// bool PlannerBase::plan(start, goal) (robot.hpp:123, poly_map_planner_node.cpp): on the device, through mplx_poly_*
  bool plan(const Waypoint<Dim> &start, const Waypoint<Dim> &goal) override {
    if (this->planner_verbose_) { start.print("Start:"); goal.print("Goal:"); }
    this->traj_ = Trajectory<Dim>();
    this->traj_cost_ = std::numeric_limits<decimal_t>::infinity();
    res_ = mplx_result();
    space_ = mplx_shim::Poly2Space();
    plan_epoch_ = 0;
    space_control_ = (int32_t)start.control & 15;
    if (Dim == 3 && has_map_) return plan3(start, goal);
    if (Dim != 2 || !has_map_) {
      printf(ANSI_COLOR_RED "[PolyMapPlanner] plan() refused: the mplx back-end plans 2-D moving-obstacle searches after setMap()\n" ANSI_COLOR_RESET);
      return false;
    }
    mplx_poly *p = shared_poly_device();
    if (!p) return false;
    const int32_t control = (int32_t)start.control & 15;
    if (!upload(p, control)) return false;
    double s9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 2; i++) {
      s9[i] = start.pos(i); s9[2 + i] = start.vel(i); s9[4 + i] = start.acc(i); s9[6 + i] = start.jrk(i);
      g9[i] = goal.pos(i); g9[2 + i] = goal.vel(i); g9[4 + i] = goal.acc(i); g9[6 + i] = goal.jrk(i);
    }
    s9[8] = start.t;
    const int32_t world = 0;
    uint64_t *cap = shared_poly_capacity();
    if (this->use_lpastar_) return plan_lpastar(start, s9, g9, control);
    if (!check(p, mplx_poly_set_record(p, 1u << 20))) return false;  // (expansion order of the first 2^20 expansions: getExpandedNodes)
    for (int attempt = 0;; attempt++) {
      if (!check(p, mplx_poly_set_capacity(p, 1, cap[0], cap[1], cap[2]))) return false;
      if (!check(p, mplx_poly_plan_batch(p, 1, &world, s9, g9, this->epsilon_, this->tol_pos_, this->tol_vel_, this->max_num_,
                                         this->heur_ignore_dynamics_ ? 1 : 0, &res_))) return false;
      if (res_.status != MPLX_PLAN_POOL_FULL || attempt >= 6) break;
      for (int k = 0; k < 3; k++) cap[k] *= 2;  // (the reference grows std containers: grow the device pools and search again)
      printf(ANSI_COLOR_CYAN "[PolyMapPlanner] device pools exhausted: doubled, planning again\n" ANSI_COLOR_RESET);
    }
    plan_epoch_ = mplx_poly_plan_epoch(p);  // (the getters answer while this is still the device object's last plan)
    if (res_.status == MPLX_PLAN_START_OCCUPIED) { printf(ANSI_COLOR_RED "[PlannerBase] start is not free!\n" ANSI_COLOR_RESET); return false; }
    this->traj_cost_ = res_.cost;
    if (res_.status != MPLX_PLAN_OK || std::isinf(res_.cost)) {
      printf(ANSI_COLOR_RED "[MPPlanner] Cannot find a traj! (status %d)\n" ANSI_COLOR_RESET, res_.status);
      this->traj_cost_ = std::numeric_limits<decimal_t>::infinity();
      return false;
    }
    const int len = res_.traj_len;
    std::vector<int32_t> actions((size_t)(len > 0 ? len : 1)), ids((size_t)len + 1);
    std::vector<double> states((size_t)(len + 1) * 9);
    if (!check(p, mplx_poly_result_traj(p, 0, actions.data(), ids.data(), states.data()))) return false;
    vec_E<Primitive<Dim>> prs;
    for (int i = 0; i < len; i++) {
      Waypoint<Dim> w(start.control);
      const double *s = &states[(size_t)i * 9];
      for (int k = 0; k < 2; k++) { w.pos(k) = s[k]; w.vel(k) = s[2 + k]; w.acc(k) = s[4 + k]; w.jrk(k) = s[6 + k]; }
      w.t = s[8];
      prs.push_back(Primitive<Dim>(w, this->U_vec_[(size_t)actions[(size_t)i]], this->dt_));
    }
    this->traj_ = Trajectory<Dim>(prs);
    return true;
  }
  const mplx_result &getResult() const { return res_; }
  size_t getExpandedNum() const { return (size_t)res_.n_expanded; }
  /// setLPAstar(true) on a 3-D planner is refused (there is no 3-D LPA* on the device): plan() then fails
  void setLPAstar(bool use_lpastar) {
    if (Dim == 3 && use_lpastar) refuse3("setLPAstar(true)");
    Base::setLPAstar(use_lpastar);
  }
  /// the state space / expansion order of the last plan, from the device.  2-D: positions in id order (upstream walks its hash
  /// map hm_: the order of its sets is unspecified), the expanded states in expansion order; a failed plan's sets too
  /// (poly_map_planner_node.cpp:105)
  vec_Vecf<Dim> getCloseSet() const override { return Dim == 3 ? set3(1) : set2(1, "getCloseSet()"); }
  vec_Vecf<Dim> getOpenSet() const override { return Dim == 3 ? set3(0) : set2(0, "getOpenSet()"); }
  vec_Vecf<Dim> getExpandedNodes() const override {
    if (Dim != 3) return set2(2, "getExpandedNodes()");
    vec_Vecf<Dim> ps;
    for (int32_t id : plan3_.expanded) ps.push_back(pos3((size_t)id));
    return ps;
  }
  /// Primitive(parent state, U[action], dt) of every predecessor record with finite cost / of every record, the blocked ones
  /// included (poly_map_replanner_node.cpp:184,234).  3-D: the same, from the records of the planner's last device plan (a planner
  /// that has not planned on the device, or whose plan another planner has replaced since, is refused and returns nothing).
  vec_E<Primitive<Dim>> getValidPrimitives() const override { return primitives2(false, "getValidPrimitives()"); }
  vec_E<Primitive<Dim>> getAllPrimitives() const override { return primitives2(true, "getAllPrimitives()"); }

 protected:
  void refuse3(const char *what) const {
    printf(ANSI_COLOR_RED "[PolyMapPlanner] %s refused: the mplx back-end has no 3-D LPA* (PolyMapPlanner3D plans with A* only)\n" ANSI_COLOR_RESET, what);
  }
  /// the 2-D state space of the last plan on the host (poly2_space.h), fetched at the first getter that asks; false: nothing to serve
  bool space2(bool with_blocked, const char *what) const {
    if (Dim != 2) return false;
    if (this->use_lpastar_) return lpa_ && mplx_shim::poly2_space_fetch_lpa(lpa_, res_, space_);
    if (plan_epoch_ == 0) return false;  // (no plan of this planner ran on the device: empty sets, as upstream before plan())
    return mplx_shim::poly2_space_fetch(shared_poly_device(), 0, plan_epoch_, res_, with_blocked, space_, what);
  }
  vec_Vecf<Dim> set2(int which, const char *what) const {
    vec_Vecf<Dim> ps;
    if (!space2(false, what)) return ps;
    const std::vector<double> xy = space_.positions(which);
    for (size_t i = 0; i + 1 < xy.size(); i += 2) {
      Vecf<Dim> p = Vecf<Dim>::Zero();
      p(0) = xy[i]; p(1) = xy[i + 1];
      ps.push_back(p);
    }
    return ps;
  }
  vec_E<Primitive<Dim>> primitives2(bool all, const char *what) const {
    vec_E<Primitive<Dim>> prs;
    if (Dim == 3) return primitives3(all, what);
    if (!space2(all, what)) return prs;
    auto add = [&](int32_t parent, int32_t action) {
      if (parent < 0 || (size_t)parent >= space_.n_nodes() || action < 0 || (size_t)action >= this->U_vec_.size()) return;
      const double *st = &space_.states[(size_t)parent * 9];
      Waypoint<Dim> w((Control::Control)space_control_);
      for (int k = 0; k < 2; k++) { w.pos(k) = st[k]; w.vel(k) = st[2 + k]; w.acc(k) = st[4 + k]; w.jrk(k) = st[6 + k]; }
      w.t = st[8];
      prs.push_back(Primitive<Dim>(w, this->U_vec_[(size_t)action], this->dt_));
    };
    for (size_t i = 0; i < space_.parent.size(); i++) add(space_.parent[i], space_.action[i]);
    if (all)
      for (size_t i = 0; i < space_.blocked_parent.size(); i++) add(space_.blocked_parent[i], space_.blocked_action[i]);
    return prs;
  }
  /// the 3-D counterpart, in the same order: the finite records in push_back order, then -- when `all` -- the blocked ones
  vec_E<Primitive<Dim>> primitives3(bool all, const char *what) const {
    vec_E<Primitive<Dim>> prs;
    if (!mplx_shim::poly3_space_fetch(plan3_.epoch, res_, all, space3_, what)) return prs;
    auto add = [&](int32_t parent, int32_t action) {
      if (parent < 0 || (size_t)parent >= space3_.n_nodes() || action < 0 || (size_t)action >= this->U_vec_.size()) return;
      const double *st = &space3_.states[(size_t)parent * 13];
      Waypoint<Dim> w((Control::Control)space_control_);
      for (int k = 0; k < Dim && k < 3; k++) { w.pos(k) = st[k]; w.vel(k) = st[3 + k]; w.acc(k) = st[6 + k]; w.jrk(k) = st[9 + k]; }
      w.t = st[12];
      prs.push_back(Primitive<Dim>(w, this->U_vec_[(size_t)action], this->dt_));
    };
    for (size_t i = 0; i < space3_.parent.size(); i++) add(space3_.parent[i], space3_.action[i]);
    if (all)
      for (size_t i = 0; i < space3_.blocked_parent.size(); i++) add(space3_.blocked_parent[i], space3_.blocked_action[i]);
    return prs;
  }
  Vecf<Dim> pos3(size_t id) const {
    Vecf<Dim> p;
    for (int k = 0; k < Dim && k < 3; k++) p(k) = plan3_.node_pos[3 * id + (size_t)k];
    return p;
  }
  vec_Vecf<Dim> set3(int closed) const {  // closed states, or the states in OPEN (opened and not closed)
    vec_Vecf<Dim> ps;
    for (size_t i = 0; i < plan3_.closed.size(); i++)
      if (closed ? plan3_.closed[i] != 0 : (plan3_.opened[i] != 0 && plan3_.closed[i] == 0)) ps.push_back(pos3(i));
    return ps;
  }
  static void planes3(const Polyhedron<Dim> &poly, std::vector<double> &hp) {  // n_hp x {px, py, pz, nx, ny, nz}
    hp.clear();
    for (const auto &v : poly.hyperplanes()) {
      for (int k = 0; k < 3; k++) hp.push_back(k < Dim ? v.p_(k) : 0.0);
      for (int k = 0; k < 3; k++) hp.push_back(k < Dim ? v.n_(k) : 0.0);
    }
  }
  template <class V>
  static void put3(const V &x, double *o) { for (int k = 0; k < 3; k++) o[k] = k < Dim ? x(k) : 0.0; }
  /// plan() of a 3-D planner: the world as the setters received it, planned through poly3_device.h; getTraj from the parent
  /// state and action of every step, as the 2-D path builds it
  bool plan3(const Waypoint<Dim> &start, const Waypoint<Dim> &goal) {
    plan3_ = mplx_shim::Poly3Plan();
    space3_ = mplx_shim::Poly3Space();
    if (this->use_lpastar_) {
      refuse3("plan() with setLPAstar(true)");
      return false;
    }
    mplx_shim::Poly3Query q;
    q.control = (int)start.control & 15;
    for (const auto &u : this->U_vec_)
      for (int k = 0; k < 3; k++) q.U.push_back(k < Dim && k < (int)u.rows() ? u(k) : 0.0);
    q.dt = this->dt_; q.v_max = this->v_max_; q.a_max = this->a_max_; q.j_max = this->j_max_; q.w = this->w_;
    put3(ori_, q.ori);
    put3(dim_, q.dim);
    q.start_t = start_t_;
    for (const auto &o : static_obs_) {
      mplx_shim::Poly3Obstacle d;
      d.kind = 0;
      planes3(o.geometry(), d.hp);
      put3(o.p(), d.p);
      q.obstacles.push_back(d);
    }
    for (const auto &o : linear_obs_) {
      mplx_shim::Poly3Obstacle d;
      d.kind = 1;
      planes3(o.geometry(), d.hp);
      put3(o.p(), d.p);
      put3(o.v(), d.v);
      d.cov_v = o.cov_v();
      q.obstacles.push_back(d);
    }
    for (const auto &o : nonlinear_obs_) {
      mplx_shim::Poly3Obstacle d;
      d.kind = 2;
      planes3(o.geometry(), d.hp);
      for (const auto &pr : o.traj().getPrimitives()) {  // n_seg x {cx[6], cy[6], cz[6], T}
        for (int ax = 0; ax < 3; ax++) {
          const Vec6f c = ax < Dim ? pr.pr(ax).coeff() : Vec6f();
          for (int k = 0; k < 6; k++) d.segs.push_back(c(k));
        }
        d.segs.push_back(pr.t());
      }
      d.start_t = o.start_t();
      d.dis_front = o.disappear_front_;
      d.dis_back = o.disappear_back_;
      q.obstacles.push_back(d);
    }
    put3(start.pos, q.start); put3(start.vel, q.start + 3); put3(start.acc, q.start + 6); put3(start.jrk, q.start + 9);
    q.start[12] = start.t;
    put3(goal.pos, q.goal); put3(goal.vel, q.goal + 3); put3(goal.acc, q.goal + 6); put3(goal.jrk, q.goal + 9);
    q.eps = this->epsilon_; q.tol_pos = this->tol_pos_; q.tol_vel = this->tol_vel_;
    q.max_num = this->max_num_;
    q.heur_ignore_dynamics = this->heur_ignore_dynamics_ ? 1 : 0;
    if (!mplx_shim::poly3_plan(q, plan3_)) return false;
    res_ = plan3_.res;
    if (res_.status == MPLX_PLAN_START_OCCUPIED) { printf(ANSI_COLOR_RED "[PlannerBase] start is not free!\n" ANSI_COLOR_RESET); return false; }
    this->traj_cost_ = res_.cost;
    if (res_.status != MPLX_PLAN_OK || std::isinf(res_.cost)) {
      printf(ANSI_COLOR_RED "[MPPlanner] Cannot find a traj! (status %d)\n" ANSI_COLOR_RESET, res_.status);
      this->traj_cost_ = std::numeric_limits<decimal_t>::infinity();
      return false;
    }
    vec_E<Primitive<Dim>> prs;
    for (size_t i = 0; i < plan3_.actions.size(); i++) {
      Waypoint<Dim> w(start.control);
      const double *s = &plan3_.states[i * 13];
      for (int k = 0; k < Dim && k < 3; k++) { w.pos(k) = s[k]; w.vel(k) = s[3 + k]; w.acc(k) = s[6 + k]; w.jrk(k) = s[9 + k]; }
      w.t = s[12];
      prs.push_back(Primitive<Dim>(w, this->U_vec_[(size_t)plan3_.actions[i]], this->dt_));
    }
    this->traj_ = Trajectory<Dim>(prs);
    return true;
  }
  static std::vector<double> planes(const Polyhedron<Dim> &poly) {  // n_hp x {px, py, nx, ny}
    std::vector<double> hp;
    for (const auto &v : poly.hyperplanes()) { hp.push_back(v.p_(0)); hp.push_back(v.p_(1)); hp.push_back(v.n_(0)); hp.push_back(v.n_(1)); }
    return hp;
  }
  /// the world this planner sees -- bounding box, start time, the three obstacle kinds -- as world 0 of the shared device object
  bool upload(mplx_poly *p, int32_t control) {
    std::vector<double> U;
    for (const auto &u : this->U_vec_) { U.push_back(u(0)); U.push_back(u(1)); }
    const int n_u = (int)this->U_vec_.size();
    if (!check(p, mplx_poly_config(p, control, n_u, U.data(), this->dt_, this->v_max_, this->a_max_, this->j_max_, this->w_))) return false;
    if (!check(p, mplx_poly_begin(p, 1))) return false;
    const double ori[2] = {ori_(0), ori_(1)}, dim[2] = {dim_(0), dim_(1)};
    if (!check(p, mplx_poly_set_world(p, 0, ori, dim, start_t_))) return false;
    for (const auto &o : static_obs_) {
      const std::vector<double> hp = planes(o.geometry());
      const double pt[2] = {o.p()(0), o.p()(1)};
      if (!check(p, mplx_poly_add_static(p, 0, (int32_t)(hp.size() / 4), hp.data(), pt))) return false;
    }
    for (const auto &o : linear_obs_) {
      const std::vector<double> hp = planes(o.geometry());
      const double pt[2] = {o.p()(0), o.p()(1)}, v[2] = {o.v()(0), o.v()(1)};
      if (!check(p, mplx_poly_add_linear(p, 0, (int32_t)(hp.size() / 4), hp.data(), pt, v, o.cov_v()))) return false;
    }
    for (const auto &o : nonlinear_obs_) {
      const std::vector<double> hp = planes(o.geometry());
      std::vector<double> segs;  // n_seg x {cx[6], cy[6], T}
      for (const auto &pr : o.traj().getPrimitives()) {
        for (int ax = 0; ax < 2; ax++) {
          const Vec6f c = pr.pr(ax).coeff();
          for (int k = 0; k < 6; k++) segs.push_back(c(k));
        }
        segs.push_back(pr.t());
      }
      if (!check(p, mplx_poly_add_nonlinear(p, 0, (int32_t)(hp.size() / 4), hp.data(), (int32_t)(segs.size() / 13), segs.data(), o.start_t(),
                                            o.disappear_front_ ? 1 : 0, o.disappear_back_ ? 1 : 0))) return false;
    }
    return check(p, mplx_poly_commit(p));
  }
  /// plan() with setLPAstar(true): on the planner's own device-resident state space (mplx_plpa_*)
  bool plan_lpastar(const Waypoint<Dim> &start, const double *s9, const double *g9, int32_t control) {
    if (!lpa_) {
      if (mplx_plpa_create(shared_poly_device(), &lpa_) != MPLX_OK) { lpa_ = nullptr; return false; }
      const uint64_t *cap = shared_poly_capacity();
      mplx_plpa_set_capacity(lpa_, cap[0] / 4, cap[1] / 4, cap[2] / 2);
    }
    lpa_control_ = control;
    if (!lcheck(mplx_plpa_plan(lpa_, 0, s9, g9, this->epsilon_, this->tol_pos_, this->tol_vel_, this->max_num_, this->heur_ignore_dynamics_ ? 1 : 0, &res_))) return false;
    if (res_.status == MPLX_PLAN_START_OCCUPIED) { printf(ANSI_COLOR_RED "[PlannerBase] start is not free!\n" ANSI_COLOR_RESET); return false; }
    this->traj_cost_ = res_.cost;
    if (res_.status != MPLX_PLAN_OK || std::isinf(res_.cost)) {
      printf(ANSI_COLOR_RED "[MPPlanner] Cannot find a traj! (status %d)\n" ANSI_COLOR_RESET, res_.status);
      this->traj_cost_ = std::numeric_limits<decimal_t>::infinity();
      return false;
    }
    const int len = mplx_plpa_traj_len(lpa_);
    std::vector<int32_t> actions((size_t)(len > 0 ? len : 1)), ids((size_t)len + 1);
    std::vector<double> states((size_t)(len + 1) * 9);
    if (!lcheck(mplx_plpa_result_traj(lpa_, actions.data(), ids.data(), states.data()))) return false;
    vec_E<Primitive<Dim>> prs;
    for (int i = 0; i < len; i++) {
      Waypoint<Dim> w(start.control);
      const double *s = &states[(size_t)i * 9];
      for (int k = 0; k < 2; k++) { w.pos(k) = s[k]; w.vel(k) = s[2 + k]; w.acc(k) = s[4 + k]; w.jrk(k) = s[6 + k]; }
      w.t = s[8];
      prs.push_back(Primitive<Dim>(w, this->U_vec_[(size_t)actions[(size_t)i]], this->dt_));
    }
    this->traj_ = Trajectory<Dim>(prs);
    return true;
  }
  bool lcheck(int rc) {
    if (rc == MPLX_OK) return true;
    printf(ANSI_COLOR_RED "[PolyMapPlanner] %s\n" ANSI_COLOR_RESET, mplx_plpa_last_error(lpa_));
    return false;
  }
  static bool check(mplx_poly *p, int rc) {
    if (rc == MPLX_OK) return true;
    printf(ANSI_COLOR_RED "[PolyMapPlanner] %s\n" ANSI_COLOR_RESET, mplx_poly_last_error(p));
    return false;
  }
  std::shared_ptr<PolyMapUtil<Dim>> map_util_;
  vec_E<Primitive<Dim>> blocked_prs_;
  vec_E<Primitive<Dim>> cleared_prs_;
  vec_E<PolyhedronObstacle<Dim>> static_obs_;
  vec_E<PolyhedronLinearObstacle<Dim>> linear_obs_;
  vec_E<PolyhedronNonlinearObstacle<Dim>> nonlinear_obs_;
  Vecf<Dim> ori_, dim_;
  decimal_t start_t_ = 0;
  bool has_map_ = false;
  mplx_result res_ = mplx_result();
  mplx_plpa *lpa_ = nullptr;  // the LPA* state space of this planner (setLPAstar(true)), created by its first plan()
  int32_t lpa_control_ = MPLX_ACC;
  mutable mplx_shim::Poly2Space space_;  // the 2-D state space of the last plan, fetched by the first getter that asks
  uint64_t plan_epoch_ = 0;             // mplx_poly_plan_epoch of the shared device object right after this planner's A* plan (0: none)
  int32_t space_control_ = MPLX_ACC;
  mplx_shim::Poly3Plan plan3_;  // what the last 3-D plan left on the host (trajectory, state space, expansion order)
  mutable mplx_shim::Poly3Space space3_;  // the predecessor records of the last 3-D plan, fetched by the first primitives getter that asks
};

typedef PolyMapPlanner<2> PolyMapPlanner2D;
typedef PolyMapPlanner<3> PolyMapPlanner3D;

}  // namespace MPL
#endif
