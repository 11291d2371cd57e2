/**
 * @file ellipsoid_planner.h  (mplx shim of <mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h>)
 *
 * MPL::EllipsoidPlanner: the reference's point-cloud planner (EllipsoidPlanner + env_cloud + EllipsoidUtil), as
 * mpl_test_node/src/ellipsoid_planner_node.cpp:64-175 drives it: the constructor, setMap(obs, r, ori, dim), the setters of
 * PlannerBase, plan(start, goal), getTraj / getTrajCost / getCloseSet / getOpenSet.  The cloud is indexed and the search
 * runs on the device (mplx_cloud_*, include/mplx.h); no PCL kd-tree and no host env_cloud are involved.
 * getExpandedNodes() stays empty, as upstream's (env_cloud.h:57 does not record the expanded nodes).
 * getValidPrimitives / getAllPrimitives are served from the device's state-space export (mplx_cloud_result_space*).
 * setPriorTrajectory (ellipsoid_planner_node.cpp:135) samples the trajectory on the host (P1 of csrc/mplx_cloud.h) and the
 * device search aims its heuristic at the samples (mplx_cloud_set_prior).  Requests this back-end does not cover --
 * setLPAstar(true), a prior trajectory without segments or duration -- make plan() fail with a message.
 */
#ifndef MPLX_SHIM_ELLIPSOID_PLANNER_H
#define MPLX_SHIM_ELLIPSOID_PLANNER_H
#include <mpl_planner/common/planner_base.h>
#include <mplx.h>

#include <cmath>
#include <limits>
#include <vector>

namespace MPL {

/**
 * @brief Motion primitive planner using point cloud
 */
class EllipsoidPlanner : public PlannerBase<3, Waypoint3D> {
 public:
  /**
   * @brief Simple constructor
   * @param verbose enable print out
   */
  EllipsoidPlanner(bool verbose) {
    planner_verbose_ = verbose;
    if (planner_verbose_) printf(ANSI_COLOR_CYAN "[EllipsoidPlanner] PLANNER VERBOSE ON (mplx back-end)" ANSI_COLOR_RESET "\n");
  }
  ~EllipsoidPlanner() {
    if (dev_) mplx_cloud_destroy(dev_);
  }
  EllipsoidPlanner(const EllipsoidPlanner &) = delete;
  EllipsoidPlanner &operator=(const EllipsoidPlanner &) = delete;

  /// Set map util: env_cloud(obs, r, ori, dim) -- the cloud goes to the device, which builds its index
  void setMap(const vec_Vec3f &obs, decimal_t r, const Vec3f &ori, const Vec3f &dim) {
    has_map_ = false;
    if (!device()) return;
    std::vector<double> pts(3 * obs.size());
    for (size_t i = 0; i < obs.size(); i++)
      for (int k = 0; k < 3; k++) pts[3 * i + k] = obs[i](k);
    const double o[3] = {ori(0), ori(1), ori(2)}, d[3] = {dim(0), dim(1), dim(2)};
    has_map_ = check(mplx_cloud_set_map(dev_, (int32_t)obs.size(), pts.empty() ? nullptr : pts.data(), r, o, d));
  }

  /// env_base::set_prior_trajectory with the dt and w in force (the node calls it after setDt and setW): for (t = 0;
  /// t < T; t += dt) prior.push_back({traj.evaluate(t), w (T - t)}).  The node guards an empty trajectory itself
  /// (ellipsoid_planner_node.cpp:132); one that reaches this call is refused.
  void setPriorTrajectory(const Trajectory<3> &traj) override {
    prior_state_.clear();
    prior_control_.clear();
    prior_ctg_.clear();
    const decimal_t T = traj.getTotalTime();
    if (traj.segs.empty() || !(T > 0) || !(dt_ > 0)) {
      printf(ANSI_COLOR_RED "[EllipsoidPlanner] setPriorTrajectory: prior trajectories are not supported by the mplx back-end; plan() will fail" ANSI_COLOR_RESET "\n");
      unsupported_ = true;
      return;
    }
    unsupported_ = false;
    for (decimal_t t = 0; t < T; t += dt_) {
      const Waypoint3D p = traj.evaluate(t);
      for (int k = 0; k < 3; k++) prior_state_.push_back(p.pos(k));
      for (int k = 0; k < 3; k++) prior_state_.push_back(p.vel(k));
      for (int k = 0; k < 3; k++) prior_state_.push_back(p.acc(k));
      for (int k = 0; k < 3; k++) prior_state_.push_back(p.jrk(k));
      prior_state_.push_back(t);
      prior_control_.push_back((int32_t)p.control & 15);
      prior_ctg_.push_back(w_ * (T - t));
    }
  }

  /// PlannerBase::plan(start, goal) (ellipsoid_planner_node.cpp:162): on the device, through mplx_cloud_*
  bool plan(const Waypoint3D &start, const Waypoint3D &goal) override {
    if (planner_verbose_) { start.print("Start:"); goal.print("Goal:"); }
    traj_ = Trajectory<3>();
    traj_cost_ = std::numeric_limits<decimal_t>::infinity();
    close_.clear();
    open_.clear();
    res_ = mplx_result();
    planned_ = false;
    if (use_lpastar_) {
      printf(ANSI_COLOR_RED "[EllipsoidPlanner] plan() refused: LPA* is not supported by the point-cloud back-end" ANSI_COLOR_RESET "\n");
      return false;
    }
    if (unsupported_) {
      printf(ANSI_COLOR_RED "[EllipsoidPlanner] plan() refused: a prior trajectory was set, which the mplx back-end does not support" ANSI_COLOR_RESET "\n");
      return false;
    }
    if (!has_map_ || U_vec_.empty()) {
      printf(ANSI_COLOR_RED "[EllipsoidPlanner] plan() refused: setMap() and setU() come first" ANSI_COLOR_RESET "\n");
      return false;
    }
    const int32_t control = (int32_t)start.control & 15;
    std::vector<double> U(3 * U_vec_.size());
    for (size_t i = 0; i < U_vec_.size(); i++)
      for (int k = 0; k < 3; k++) U[3 * i + k] = U_vec_[i](k);
    if (!check(mplx_cloud_config(dev_, control, (int32_t)U_vec_.size(), U.data(), dt_, v_max_, a_max_, j_max_, w_))) return false;
    {  // the prior in force (none: cleared), for this and the later plans
      const int32_t off[2] = {0, (int32_t)prior_ctg_.size()};
      const int32_t n_sets = prior_ctg_.empty() ? 0 : 1;
      if (!check(mplx_cloud_set_prior(dev_, n_sets, off, prior_state_.data(), prior_control_.data(), prior_ctg_.data()))) return false;
    }
    double s[13], g[13];
    for (int k = 0; k < 3; k++) {
      s[k] = start.pos(k); s[3 + k] = start.vel(k); s[6 + k] = start.acc(k); s[9 + k] = start.jrk(k);
      g[k] = goal.pos(k); g[3 + k] = goal.vel(k); g[6 + k] = goal.acc(k); g[9 + k] = goal.jrk(k);
    }
    s[12] = start.t;
    g[12] = goal.t;
    for (int attempt = 0;; attempt++) {
      if (!check(mplx_cloud_set_capacity(dev_, 1, cap_[0], cap_[1], cap_[2]))) return false;
      if (!check(mplx_cloud_plan_batch(dev_, 1, s, g, epsilon_, tol_pos_, tol_vel_, tol_acc_, max_num_, heur_ignore_dynamics_ ? 1 : 0, &res_)))
        return false;
      // the lattice, dt and control kind this state space was built with: what getValidPrimitives / getAllPrimitives rebuild from
      plan_U_ = U_vec_;
      plan_dt_ = dt_;
      plan_control_ = start.control;
      planned_ = true;
      if (res_.status != MPLX_PLAN_POOL_FULL || attempt >= 6) break;
      for (int k = 0; k < 3; k++) cap_[k] *= 2;  // (the reference grows std containers: grow the device pools and search again)
      printf(ANSI_COLOR_CYAN "[EllipsoidPlanner] device pools exhausted: doubled, planning again" ANSI_COLOR_RESET "\n");
    }
    // the state space: getCloseSet (closed) and getOpenSet (opened, not closed)
    const size_t n = (size_t)res_.n_nodes;
    if (n > 0) {
      std::vector<mplx_waypoint> coords(n);
      std::vector<int32_t> closed(n), opened(n);
      if (!check(mplx_cloud_result_nodes(dev_, 0, n, coords.data(), nullptr, closed.data(), opened.data()))) return false;
      for (size_t i = 0; i < n; i++) {
        const Vec3f p(coords[i].pos[0], coords[i].pos[1], coords[i].pos[2]);
        if (closed[i]) close_.push_back(p);
        else if (opened[i]) open_.push_back(p);
      }
    }
    if (res_.status != MPLX_PLAN_OK || std::isinf(res_.cost)) {
      printf(ANSI_COLOR_RED "[MPPlanner] Cannot find a traj! (status %d)" ANSI_COLOR_RESET "\n", res_.status);
      return false;
    }
    traj_cost_ = res_.cost;
    const int len = res_.traj_len;
    if (len > 0) {
      std::vector<mplx_waypoint> wps((size_t)len + 1);
      std::vector<int32_t> actions((size_t)len), ids((size_t)len + 1);
      if (!check(mplx_cloud_result_traj(dev_, 0, wps.data(), actions.data(), ids.data()))) return false;
      vec_E<Primitive<3>> prs;
      for (int i = 0; i < len; i++) {  // forward_action(parent, action): the primitive from the stored parent state
        Waypoint3D w(start.control);
        for (int k = 0; k < 3; k++) { w.pos(k) = wps[(size_t)i].pos[k]; w.vel(k) = wps[(size_t)i].vel[k]; w.acc(k) = wps[(size_t)i].acc[k]; w.jrk(k) = wps[(size_t)i].jrk[k]; }
        w.t = wps[(size_t)i].t;
        prs.push_back(Primitive<3>(w, U_vec_[(size_t)actions[(size_t)i]], dt_));
      }
      traj_ = Trajectory<3>(prs);
    }
    return true;
  }

  vec_Vec3f getCloseSet() const override { return close_; }
  vec_Vec3f getOpenSet() const override { return open_; }
  /// empty, as the reference's: env_cloud::get_succ does not record expanded nodes (env_cloud.h:57)
  vec_Vec3f getExpandedNodes() const override { return vec_Vec3f(); }
  const mplx_result &getResult() const { return res_; }
  /// PlannerBase::getValidPrimitives / getAllPrimitives: Primitive<3>(parent state, U[action], dt) of every predecessor record of
  /// the last plan's state space, in record order (for every state in id order its records in arrival order), with the U and dt
  /// in force at that plan().  States and records come from the device export (mplx_cloud_result_space / _edges of query 0).
  /// Both return the same list: env_cloud::get_succ SKIPS blocked primitives and never emits them with cost +inf (mplx.h, the
  /// point-cloud section), so the state space holds no record that is not valid.  Empty when nothing was planned or the plan
  /// failed before the device; a refused export prints its message.
  vec_E<Primitive<3>> getValidPrimitives() const override { return device_primitives(); }
  vec_E<Primitive<3>> getAllPrimitives() const override { return device_primitives(); }

 private:
  vec_E<Primitive<3>> device_primitives() const {
    vec_E<Primitive<3>> prs;
    if (!dev_ || !planned_) return prs;
    const int32_t q = 0;
    uint64_t node_off[2] = {0, 0}, edge_off[2] = {0, 0};
    if (!report(mplx_cloud_result_space_counts(dev_, 1, &q, node_off, edge_off))) return prs;
    const size_t n = (size_t)node_off[1], m = (size_t)edge_off[1];
    if (n == 0 || m == 0) return prs;
    std::vector<double> st(13 * n);
    std::vector<int32_t> parent(m), action(m);
    if (!report(mplx_cloud_result_space(dev_, 1, &q, n, st.data(), nullptr, nullptr, nullptr, nullptr))) return prs;
    if (!report(mplx_cloud_result_space_edges(dev_, 1, &q, m, nullptr, parent.data(), action.data()))) return prs;
    for (size_t i = 0; i < m; i++) {
      const double *s = &st[13 * (size_t)parent[i]];
      Waypoint3D w(plan_control_);
      for (int k = 0; k < 3; k++) { w.pos(k) = s[k]; w.vel(k) = s[3 + k]; w.acc(k) = s[6 + k]; w.jrk(k) = s[9 + k]; }
      w.t = s[12];
      prs.push_back(Primitive<3>(w, plan_U_[(size_t)action[i]], plan_dt_));
    }
    return prs;
  }
  bool report(int code) const {
    if (code == MPLX_OK) return true;
    printf(ANSI_COLOR_RED "[EllipsoidPlanner] %s" ANSI_COLOR_RESET "\n", mplx_cloud_last_error(dev_));
    return false;
  }
  bool device() {
    if (dev_) return true;
    if (mplx_cloud_create(0, &dev_) != MPLX_OK) {
      printf(ANSI_COLOR_RED "[EllipsoidPlanner] %s" ANSI_COLOR_RESET "\n", mplx_cloud_last_error(nullptr));
      dev_ = nullptr;
      return false;
    }
    return true;
  }
  bool check(int code) {
    if (code == MPLX_OK) return true;
    printf(ANSI_COLOR_RED "[EllipsoidPlanner] %s" ANSI_COLOR_RESET "\n", mplx_cloud_last_error(dev_));
    return false;
  }

  mplx_cloud *dev_ = nullptr;
  bool has_map_ = false;
  mplx_result res_ = mplx_result();
  std::vector<double> prior_state_, prior_ctg_;  // the sampled prior trajectory: 13 doubles and a cost-to-go per entry
  std::vector<int32_t> prior_control_;
  vec_Vec3f close_, open_;
  bool planned_ = false;  // the device holds the state space of the last plan()
  vec_E<VecDf> plan_U_;
  decimal_t plan_dt_ = 1.0;
  Control::Control plan_control_ = Control::NONE;
  uint64_t cap_[3] = {1u << 20, 1u << 22, 1u << 21};  // pool capacities: states, predecessor records, OPEN-log entries
};
}  // namespace MPL

#endif
