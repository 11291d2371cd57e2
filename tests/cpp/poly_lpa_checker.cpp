// tests/cpp/poly_lpa_checker.cpp -- CPU checker of the moving-obstacle LPA* at Dim = 2 and 3, compiled with g++ at test time and
// loaded through ctypes (tests/poly_lpa_checker.py).  TEST INFRASTRUCTURE ONLY.
//
// The environment is the Env<Dim> of tests/cpp/poly_checker.cpp, included as it is (its pc_* entries work on the handles made here
// too: obstacles, set-up, get_succ, the fresh best-first search).  The LPA* is the one of oracle/ref_stubs/poly_map_ref_api.cpp
// (refpoly_lpa_*), restated over that environment: PlannerBase::plan with setLPAstar(true), PolyMapPlanner::updateNodes
// (poly_map_planner.h:61-93) and getSubStateSpace as poly_map_replanner_node.cpp:123-186,231 drives them --
//   * every successor get_succ emits is a state with a predecessor entry, the blocked ones too (cost +inf); no blocked log;
//   * OPEN is rebuilt from the inconsistent states at entry, ordered by (key, min(g, rhs), id); the goal-state follow rule;
//   * updateNodes re-tests every entry of every state with Primitive(pred, U[action], dt) + isFree(pr, pred.t), collects what
//     flipped and recomputes the look-ahead value of the states whose entries changed;
//   * getSubStateSpace(k): planning afresh from the k-th state of the last trajectory;
//   * entries are numbered in creation order (expansion order, then the order get_succ emits).
// One state space per handle.  The goal test is the one of the checker's best-first search (position, and velocity with
// tol_vel >= 0); the dynamics-aware heuristic goes through the function pointer pc_set_heuristic took.  At Dim = 2 the tests pin all
// of this to refpoly_lpa_* bit for bit; at Dim = 3 it is the same template.
#include "poly_checker.cpp"

#include <algorithm>

namespace {

struct LpaIface {
  virtual ~LpaIface() {}
  int valid = 0, n_entries = 0, iterations = 0;
  double cost = INF;
  std::vector<int> lexpanded, ltraj_nodes, ltraj_act, changed_entry, changed_blocked, echild, eparent, eaction;
  virtual void clear_obstacles(double start_t) = 0;
  virtual void lpa_reset() = 0;
  virtual int lpa_plan(const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) = 0;
  virtual void lpa_update_nodes(int *n_blocked, int *n_cleared) = 0;
  virtual void lpa_sub_state_space(int k, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) = 0;
  virtual int lpa_num_nodes() const = 0;
  virtual void lpa_node(int id, double *state, double *vals, int *flags) const = 0;
  virtual void lpa_entries(int *child, int *parent, int *action, int *blocked) const = 0;
};

template <int Dim>
struct LpaChecker : Checker<Dim>, LpaIface {
  using Checker<Dim>::E;
  using Checker<Dim>::from;
  using Checker<Dim>::to;
  static const int NS = 4 * Dim + 1;
  struct LNode {
    Waypoint<Dim> coord;
    double g, rhs, h;
    int closed, opened, built;
    std::vector<int> pred, pact, pentry, pblk;
    std::vector<double> pcost;  // the intrinsic cost of the primitive, whether blocked or not
  };
  struct LEntry { double k, kg; int id; };
  std::vector<LNode> ln;
  std::map<std::vector<int>, int> table;
  int root = -1, goal_id = -1;
  double goal_[NS];

  LpaChecker() { for (int i = 0; i < NS; i++) goal_[i] = 0; }

  void clear_obstacles(double start_t) override {
    E.st.clear(); E.lin.clear(); E.nl.clear();
    E.start_t = start_t;
  }
  void lpa_reset() override {
    ln.clear(); table.clear();
    root = -1; goal_id = -1;
    valid = 0; n_entries = 0; iterations = 0; cost = INF;
    for (int i = 0; i < NS; i++) goal_[i] = 0;
    lexpanded.clear(); ltraj_nodes.clear(); ltraj_act.clear(); changed_entry.clear(); changed_blocked.clear();
    echild.clear(); eparent.clear(); eaction.clear();
  }
  double rhs_of(const LNode &nd) const {
    double rhs = INF;
    for (size_t e = 0; e < nd.pred.size(); e++) {
      if (nd.pblk[e]) continue;
      const double v = ln[nd.pred[e]].g + nd.pcost[e];
      if (v < rhs) rhs = v;
    }
    return rhs;
  }
  int lpa_plan(const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) override {
    cost = INF;
    lexpanded.clear(); ltraj_nodes.clear(); ltraj_act.clear();
    iterations = 0;
    Waypoint<Dim> s = from(start, control), g = from(goal, control);
    s.enable_t = true;
    if (!E.is_inside(s.pos)) return 2;
    if (heur_mode == 0 && !g_heur_fn) return -1;
    auto heur = [&](const Waypoint<Dim> &x) {
      if (eps == 0) return 0.0;
      if (heur_mode == 0) {
        OrcWaypoint o = OrcWaypoint();
        for (int i = 0; i < Dim; i++) { o.pos[i] = x.pos(i); o.vel[i] = x.vel(i); o.acc[i] = x.acc(i); o.jrk[i] = x.jrk(i); }
        o.t = x.t;
        o.control = control;
        o.enable_t = 1;
        return g_heur_fn(g_heur_planner, &o);
      }
      const double d = this->linf(x, g);
      return E.v_max > 0 ? E.w * d / E.v_max : E.w * d;
    };
    auto is_goal = [&](const Waypoint<Dim> &x) {
      bool ok = this->linf(x, g) <= tol_pos;
      if (ok && (control & 2) && tol_vel >= 0) {
        double d = 0;
        for (int i = 0; i < Dim; i++) d = std::max(d, std::fabs(x.vel(i) - g.vel(i)));
        ok = d <= tol_vel;
      }
      return ok;
    };
    bool same_goal = true;
    for (int i = 0; i < NS - 1; i++) same_goal = same_goal && goal_[i] == goal[i];
    if (valid && !same_goal) valid = 0;
    for (int i = 0; i < NS; i++) goal_[i] = goal[i];
    if (is_goal(s)) { cost = 0; return 0; }
    if (valid) {  // the start must be the current root
      auto f = table.find(s.key());
      if (f == table.end() || f->second != root) valid = 0;
    }
    if (!valid) {
      ln.clear(); table.clear(); echild.clear(); eparent.clear(); eaction.clear();
      n_entries = 0;
      ln.push_back(LNode{s, INF, 0.0, heur(s), 0, 1, 0, {}, {}, {}, {}, {}});
      table[s.key()] = 0;
      root = 0;
      goal_id = -1;
      valid = 1;
    }
    auto key_of = [&](const LNode &nd) { return std::min(nd.g, nd.rhs) + eps * nd.h; };
    auto later = [](const LEntry &a, const LEntry &b) { if (a.k != b.k) return a.k > b.k; if (a.kg != b.kg) return a.kg > b.kg; return a.id > b.id; };
    std::priority_queue<LEntry, std::vector<LEntry>, decltype(later)> open(later);
    auto push = [&](int id) { const LNode &nd = ln[id]; open.push(LEntry{key_of(nd), std::min(nd.g, nd.rhs), id}); };
    auto entry_valid = [&](const LEntry &e) {
      const LNode &nd = ln[e.id];
      if (nd.g == nd.rhs) return false;
      return e.k == key_of(nd) && e.kg == std::min(nd.g, nd.rhs);
    };
    auto update_node = [&](int id, bool g_changed) {
      LNode &nd = ln[id];
      const double old_rhs = nd.rhs;
      if (id != root) nd.rhs = rhs_of(nd);
      if (nd.g != nd.rhs) {
        const bool had_entry = !g_changed && nd.opened && !nd.closed && nd.rhs == old_rhs;
        nd.opened = 1;
        nd.closed = 0;
        if (!had_entry) push(id);
      } else if (nd.opened && !nd.closed) {
        nd.closed = 1;
      }
    };
    for (size_t i = 0; i < ln.size(); i++)  // OPEN = the inconsistent states, rebuilt
      if (ln[i].g != ln[i].rhs) push((int)i);
    int gid = -1;  // the goal state to follow
    for (size_t i = 0; i < ln.size(); i++) {
      const LNode &nd = ln[i];
      if (nd.g != nd.rhs || std::isinf(nd.g) || !is_goal(nd.coord)) continue;
      if (gid < 0) { gid = (int)i; continue; }
      const LNode &b = ln[gid];
      const double k = key_of(nd), kb = key_of(b);
      if (k < kb || (k == kb && nd.g < b.g)) gid = (int)i;
    }
    if (gid < 0 && goal_id >= 0 && goal_id < (int)ln.size() && is_goal(ln[goal_id].coord)) gid = goal_id;
    vec_E<Waypoint<Dim>> succ;
    std::vector<double> scost;
    std::vector<int> act;
    int status = 0;
    for (;;) {
      while (!open.empty() && !entry_valid(open.top())) open.pop();
      const bool gcons = gid < 0 || ln[gid].g == ln[gid].rhs;
      const double kgoal = gid < 0 ? INF : key_of(ln[gid]);
      if (open.empty()) {
        if (!(gid >= 0 && gcons && !std::isinf(ln[gid].g))) status = 1;
        break;
      }
      if (!(open.top().k < kgoal || !gcons)) break;
      iterations++;
      const int u = open.top().id;
      open.pop();
      ln[u].opened = 1;
      ln[u].closed = 1;
      lexpanded.push_back(u);
      if (ln[u].g > ln[u].rhs) {
        ln[u].g = ln[u].rhs;
      } else {
        ln[u].g = INF;
        update_node(u, true);
      }
      const Waypoint<Dim> cw = ln[u].coord;
      const bool first = !ln[u].built;
      E.get_succ(cw, succ, scost, act);
      std::vector<int> kids;
      for (size_t k = 0; k < succ.size(); k++) {
        Waypoint<Dim> tn = succ[k];
        tn.control = cw.control;
        auto f = table.find(tn.key());
        int id = f == table.end() ? -1 : f->second;
        if (first) {
          if (id < 0) {
            id = (int)ln.size();
            ln.push_back(LNode{tn, INF, INF, heur(tn), 0, 0, 0, {}, {}, {}, {}, {}});
            table[tn.key()] = id;
          }
          const Primitive<Dim> pr(cw, E.U[act[k]], E.dt);
          LNode &c = ln[id];
          c.pred.push_back(u); c.pact.push_back(act[k]); c.pentry.push_back(n_entries); c.pblk.push_back(std::isinf(scost[k]) ? 1 : 0);
          c.pcost.push_back(E.cost(pr));
          echild.push_back(id); eparent.push_back(u); eaction.push_back(act[k]);
          n_entries++;
        } else if (id < 0) {
          continue;
        }
        if (std::isinf(scost[k])) continue;  // (a blocked entry cannot lower the successor's look-ahead value)
        if (std::find(kids.begin(), kids.end(), id) == kids.end()) kids.push_back(id);
      }
      ln[u].built = 1;
      for (int id : kids) update_node(id, false);
      if (is_goal(ln[u].coord) && !std::isinf(ln[u].g)) gid = u;
      if (max_expand > 0 && iterations >= max_expand) { status = 3; break; }
    }
    goal_id = gid;
    if (status != 0) return status;
    // recoverTraj: minimise g(pred) + cost over the non-blocked entries, ties -> larger g(pred), then the oldest
    int node = gid;
    ltraj_nodes.push_back(node);
    while (!ln[node].pred.empty()) {
      int best = -1;
      double min_rhs = INF, min_g = INF;
      const LNode &nd = ln[node];
      for (size_t e = 0; e < nd.pred.size(); e++) {
        const double gp = ln[nd.pred[e]].g, c = nd.pblk[e] ? INF : nd.pcost[e];
        if (min_rhs > gp + c) { min_rhs = gp + c; min_g = gp; best = (int)e; }
        else if (!std::isinf(c) && min_rhs == gp + c && min_g < gp) { min_g = gp; best = (int)e; }
      }
      if (best < 0) return 1;
      ltraj_act.push_back(nd.pact[best]);
      node = nd.pred[best];
      ltraj_nodes.push_back(node);
      if (node == root) break;
      if (ltraj_nodes.size() > ln.size() + 1) return 1;
    }
    if (node != root) return 1;
    cost = ln[gid].g;
    return 0;
  }
  void lpa_update_nodes(int *n_blocked, int *n_cleared) override {
    changed_entry.clear(); changed_blocked.clear();
    int nb = 0, nc = 0;
    *n_blocked = 0; *n_cleared = 0;
    if (!valid) return;
    std::vector<int> dirty(ln.size(), 0);
    for (size_t i = 0; i < ln.size(); i++) {
      LNode &nd = ln[i];
      for (size_t e = 0; e < nd.pred.size(); e++) {
        const Waypoint<Dim> &pc = ln[nd.pred[e]].coord;
        const Primitive<Dim> pr(pc, E.U[nd.pact[e]], E.dt);
        const bool free_ = E.is_free(pr, pc.t);
        if (!free_ && !nd.pblk[e]) { nd.pblk[e] = 1; dirty[i] = 1; nb++; changed_entry.push_back(nd.pentry[e]); changed_blocked.push_back(1); }
        else if (free_ && nd.pblk[e]) { nd.pblk[e] = 0; dirty[i] = 1; nc++; changed_entry.push_back(nd.pentry[e]); changed_blocked.push_back(0); }
      }
    }
    for (size_t i = 0; i < ln.size(); i++)
      if (dirty[i] && (int)i != root) ln[i].rhs = rhs_of(ln[i]);
    *n_blocked = nb; *n_cleared = nc;
  }
  void lpa_sub_state_space(int k, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) override {
    if (!valid || ltraj_act.empty() || k < 0 || k > (int)ltraj_act.size()) return;
    const int n = (int)ltraj_act.size();
    double s[NS], goal[NS];
    to(ln[ltraj_nodes[n - k]].coord, s);  // (ltraj_nodes is goal -> start)
    for (int i = 0; i < NS; i++) goal[i] = goal_[i];
    valid = 0;
    lpa_plan(s, goal, control, eps, tol_pos, tol_vel, max_expand, heur_mode);
    lexpanded.clear(); ltraj_nodes.clear(); ltraj_act.clear();  // (not a plan: no expansion record, no trajectory of its own)
    cost = INF;
  }
  int lpa_num_nodes() const override { return (int)ln.size(); }
  void lpa_node(int id, double *state, double *vals, int *flags) const override {
    const LNode &nd = ln[id];
    to(nd.coord, state);
    vals[0] = nd.g; vals[1] = nd.rhs; vals[2] = nd.h;
    flags[0] = nd.closed; flags[1] = nd.opened; flags[2] = nd.built;
  }
  void lpa_entries(int *child, int *parent, int *action, int *blocked) const override {
    for (int e = 0; e < n_entries; e++) { child[e] = echild[e]; parent[e] = eparent[e]; action[e] = eaction[e]; blocked[e] = 0; }
    for (const LNode &nd : ln)
      for (size_t e = 0; e < nd.pred.size(); e++) blocked[nd.pentry[e]] = nd.pblk[e];
  }
};

LpaIface *lpa_of(void *h) { return dynamic_cast<LpaIface *>((Base *)h); }

}  // namespace

extern "C" {
// a checker handle with an LPA* state space of its own: every pc_* entry works on it, pc_destroy frees it
void *plc_create(int dim, const double *ori, const double *size, double start_t) {
  Base *b = nullptr;
  if (dim == 2) { auto *c = new LpaChecker<2>(); set_box(c->E, ori, size); c->E.start_t = start_t; b = c; }
  if (dim == 3) { auto *c = new LpaChecker<3>(); set_box(c->E, ori, size); c->E.start_t = start_t; b = c; }
  return b;
}
// the obstacles moved / the planner's start time changed: drop the obstacles (pc_add_* follow), set the start time
void plc_clear_obstacles(void *h, double start_t) { lpa_of(h)->clear_obstacles(start_t); }
int plc_initialized(void *h) { return lpa_of(h)->valid; }
void plc_reset(void *h) { lpa_of(h)->lpa_reset(); }
int plc_plan(void *h, const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) {
  return lpa_of(h)->lpa_plan(start, goal, control, eps, tol_pos, tol_vel, max_expand, heur_mode);
}
void plc_update_nodes(void *h, int *n_blocked, int *n_cleared) { lpa_of(h)->lpa_update_nodes(n_blocked, n_cleared); }
void plc_sub_state_space(void *h, int k, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) {
  lpa_of(h)->lpa_sub_state_space(k, control, eps, tol_pos, tol_vel, max_expand, heur_mode);
}
int plc_num_nodes(void *h) { return lpa_of(h)->lpa_num_nodes(); }
int plc_num_entries(void *h) { return lpa_of(h)->n_entries; }
int plc_iterations(void *h) { return lpa_of(h)->iterations; }
double plc_cost(void *h) { return lpa_of(h)->cost; }
int plc_traj_len(void *h) { return (int)lpa_of(h)->ltraj_act.size(); }
void plc_get_expanded(void *h, int *ids) {
  const LpaIface *l = lpa_of(h);
  for (size_t i = 0; i < l->lexpanded.size(); i++) ids[i] = l->lexpanded[i];
}
// path in start -> goal order: node ids (len + 1), actions (len)
void plc_get_traj(void *h, int *node_ids, int *actions) {
  const LpaIface *l = lpa_of(h);
  const size_t n = l->ltraj_act.size();
  for (size_t i = 0; i <= n && !l->ltraj_nodes.empty(); i++) node_ids[i] = l->ltraj_nodes[n - i];
  for (size_t i = 0; i < n; i++) actions[i] = l->ltraj_act[n - 1 - i];
}
// per state: pos vel acc jrk (Dim each) t | g rhs h | closed opened built
void plc_get_node(void *h, int id, double *state, double *vals, int *flags) { lpa_of(h)->lpa_node(id, state, vals, flags); }
// per entry, in creation order: child, parent, action, blocked
void plc_get_entries(void *h, int *child, int *parent, int *action, int *blocked) { lpa_of(h)->lpa_entries(child, parent, action, blocked); }
int plc_num_changed(void *h) { return (int)lpa_of(h)->changed_entry.size(); }
void plc_get_changed(void *h, int *entry, int *now_blocked) {
  const LpaIface *l = lpa_of(h);
  for (size_t i = 0; i < l->changed_entry.size(); i++) { entry[i] = l->changed_entry[i]; now_blocked[i] = l->changed_blocked[i]; }
}
}
