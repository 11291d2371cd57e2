// oracle/_ref/libpolymap3_ref.so -- the reference's OWN moving-obstacle environment at Dim = 3, compiled from where it lies.
//
// TEST INFRASTRUCTURE ONLY (see oracle/mpl_oracle.h).  The 3-D companion of poly_map_ref_api.cpp: the same in-tree headers
//   mpl_external_planner/include/mpl_external_planner/poly_map_planner/env_poly_map.h      (get_succ, intrinsic cost)
//   .../poly_map_planner/poly_map_util.h                                                   (six-face setBoundingBox, isInside, isFree)
//   .../poly_map_planner/primitive_geometry_utils.h                                        (the three collide())
//   .../poly_map_planner/simple_obstacle.h                                                 (static / linear / nonlinear obstacles)
// instantiated as PolyMapUtil<3> / env_poly_map<3> / Polyhedron*Obstacle3D and wrapped in a C interface; `make -C oracle ref`
// compiles it against those headers (never copied) and the stand-ins of include/mpl_shim, with the flags of libpolymap_ref.so.
// Vectors cross the interface as pointers to Dim doubles; rows are the 3-D layouts: hyperplanes {p3, n3}, segments
// {cx[6], cy[6], cz[6], T}, states pos3 vel3 acc3 jrk3 t.  What the 2-D library leaves untested by construction is what this one
// is for: the third term of every sum, the 3-D bounding box, Vec3f obstacle points and velocities.
//
// The best-first search is refpoly_plan's, line for line, over env_poly_map<3> (GraphSearch is not vendored: same restatement,
// same order, ties and recoverTraj; goal test on the position).  No LPA*: the device refuses 3-D LPA*.
#include <mpl_external_planner/poly_map_planner/poly_map_planner.h>

#include <cstring>
#include <map>
#include <queue>

namespace {
constexpr int Dim = 3, NS = 4 * Dim + 1, NSEG = 6 * Dim + 1;
typedef Vecf<Dim> Vec;
typedef Waypoint<Dim> Wp;
struct Ref {
  std::shared_ptr<PolyMapUtil<Dim>> map_util;
  std::shared_ptr<MPL::env_poly_map<Dim>> env;
  vec_E<PolyhedronObstacle<Dim>> st;
  vec_E<PolyhedronLinearObstacle<Dim>> lin;
  vec_E<PolyhedronNonlinearObstacle<Dim>> nl;
};
Vec vec_of(const double *x) {
  Vec v;
  for (int i = 0; i < Dim; i++) v(i) = x[i];
  return v;
}
Polyhedron<Dim> poly_of(int n_hp, const double *hp) {
  Polyhedron<Dim> p;
  for (int i = 0; i < n_hp; i++) p.add(Hyperplane<Dim>(vec_of(hp + 2 * Dim * i), vec_of(hp + 2 * Dim * i + Dim)));
  return p;
}
Wp wp_of(const double *s, int control) {
  Wp w((Control::Control)control);
  w.pos = vec_of(s); w.vel = vec_of(s + Dim); w.acc = vec_of(s + 2 * Dim); w.jrk = vec_of(s + 3 * Dim);
  w.t = s[4 * Dim];
  return w;
}
void wp_to(const Wp &w, double *s) {
  for (int i = 0; i < Dim; i++) { s[i] = w.pos(i); s[Dim + i] = w.vel(i); s[2 * Dim + i] = w.acc(i); s[3 * Dim + i] = w.jrk(i); }
  s[4 * Dim] = w.t;
}
void sync(Ref *r) {
  r->map_util->setStaticObstacle(r->st);
  r->map_util->setLinearObstacle(r->lin);
  r->map_util->setNonlinearObstacle(r->nl);
}
double linf(const Wp &x, const Wp &g) {
  double d = 0;
  for (int i = 0; i < Dim; i++) d = std::max(d, std::fabs(x.pos(i) - g.pos(i)));
  return d;
}
}  // namespace

extern "C" {
void *refpoly3_create(const double *ori, const double *dim) {
  Ref *r = new Ref();
  r->map_util.reset(new PolyMapUtil<Dim>());
  r->map_util->setBoundingBox(vec_of(ori), vec_of(dim));
  r->env.reset(new MPL::env_poly_map<Dim>(r->map_util));
  return r;
}
void refpoly3_destroy(void *h) { delete (Ref *)h; }
void refpoly3_set_start_time(void *h, double t) { ((Ref *)h)->map_util->setStartTime(t); }
// hp: n_hp x {p3, n3}.  The obstacle lists are handed to the map util once, by refpoly3_commit.
void refpoly3_add_static(void *h, int n_hp, const double *hp, const double *p) {
  ((Ref *)h)->st.push_back(PolyhedronObstacle<Dim>(poly_of(n_hp, hp), vec_of(p)));
}
void refpoly3_add_linear(void *h, int n_hp, const double *hp, const double *p, const double *v, double cov_v) {
  PolyhedronLinearObstacle<Dim> o(poly_of(n_hp, hp), vec_of(p), vec_of(v));
  o.set_cov_v(cov_v);
  ((Ref *)h)->lin.push_back(o);
}
// segs: n_seg x {cx[6], cy[6], cz[6], T}; the obstacle follows that trajectory from its local time start_t on
void refpoly3_add_nonlinear(void *h, int n_hp, const double *hp, int n_seg, const double *segs, int control, double start_t, int dis_front, int dis_back) {
  vec_E<Primitive<Dim>> prs;
  for (int i = 0; i < n_seg; i++) {
    vec_E<Vec6f> cs(Dim);
    for (int a = 0; a < Dim; a++)
      for (int k = 0; k < 6; k++) cs[a](k) = segs[NSEG * i + 6 * a + k];
    prs.push_back(Primitive<Dim>(cs, segs[NSEG * i + 6 * Dim], (Control::Control)control));
  }
  PolyhedronNonlinearObstacle<Dim> o(poly_of(n_hp, hp), Trajectory<Dim>(prs), start_t);
  o.disappear_front_ = dis_front != 0;
  o.disappear_back_ = dis_back != 0;
  ((Ref *)h)->nl.push_back(o);
}
void refpoly3_commit(void *h) { sync((Ref *)h); }
void refpoly3_set_env(void *h, int n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) {
  Ref *r = (Ref *)h;
  vec_E<VecDf> Us;
  for (int i = 0; i < n_u; i++) Us.push_back(vec_of(U + Dim * i));
  r->env->set_u(Us);
  r->env->set_dt(dt); r->env->set_v_max(v_max); r->env->set_a_max(a_max); r->env->set_j_max(j_max); r->env->set_w(w);
}
int refpoly3_is_inside(void *h, const double *pt) { return ((Ref *)h)->map_util->isInside(vec_of(pt)) ? 1 : 0; }
int refpoly3_is_free_point(void *h, const double *pt, double t) { return ((Ref *)h)->map_util->isFree(vec_of(pt), t) ? 1 : 0; }
// env_poly_map<3>::get_succ: out arrays sized n_u (succ: n x 13); returns the number emitted
int refpoly3_get_succ(void *h, const double *state, int control, double *succ, double *cost, int *action) {
  Ref *r = (Ref *)h;
  vec_E<Wp> s;
  std::vector<decimal_t> c;
  std::vector<int> a;
  r->env->get_succ(wp_of(state, control), s, c, a);
  for (size_t i = 0; i < s.size(); i++) { wp_to(s[i], succ + NS * i); cost[i] = c[i]; action[i] = a[i]; }
  return (int)s.size();
}

// ---- best-first search over env_poly_map<3>: refpoly_plan of poly_map_ref_api.cpp (see there for every choice).
// heur_mode != 0: w * |dp|_inf / v_max; heur_mode == 0: the oracle's orc_heuristic through refpoly3_set_heuristic.
struct PNode { Wp coord; double g, h; int closed, opened; std::vector<int> pred, pact; std::vector<double> pcost; };
static std::vector<int> g_exp, g_traj_nodes, g_traj_act;
static std::vector<PNode> g_nodes;
static double g_cost;
typedef double (*orc_heur_fn)(const void *planner, const void *waypoint);
static orc_heur_fn g_heur_fn = nullptr;
static const void *g_heur_planner = nullptr;
// layout of orc_waypoint (oracle/mpl_oracle.h)
struct OrcWaypoint { double pos[3], vel[3], acc[3], jrk[3]; double yaw, t; int32_t control, enable_t; };
void refpoly3_set_heuristic(void *fn, const void *planner) { g_heur_fn = (orc_heur_fn)fn; g_heur_planner = planner; }
int refpoly3_plan(void *h, const double *start, const double *goal, int control, double eps, double tol_pos, int max_expand, int heur_mode) {
  Ref *r = (Ref *)h;
  g_nodes.clear(); g_exp.clear(); g_traj_nodes.clear(); g_traj_act.clear();
  g_cost = std::numeric_limits<double>::infinity();
  Wp s = wp_of(start, control), g = wp_of(goal, control);
  s.enable_t = true;
  if (!r->env->is_free(s.pos)) return 2;
  const double v_max = r->env->v_max_, w = r->env->w_;
  auto heur = [&](const Wp &x) {
    if (heur_mode == 0) {
      OrcWaypoint o = OrcWaypoint();
      for (int i = 0; i < Dim; i++) { o.pos[i] = x.pos(i); o.vel[i] = x.vel(i); o.acc[i] = x.acc(i); o.jrk[i] = x.jrk(i); }
      o.t = x.t;
      o.control = control;
      o.enable_t = 1;
      return g_heur_fn(g_heur_planner, &o);
    }
    const double d = linf(x, g);
    return v_max > 0 ? w * d / v_max : w * d;
  };
  if (heur_mode == 0 && !g_heur_fn) return -1;  // refpoly3_set_heuristic first
  auto is_goal = [&](const Wp &x) { return linf(x, g) <= tol_pos; };
  if (is_goal(s)) { g_cost = 0; return 0; }
  std::map<std::vector<int>, int> table;
  struct E { double f, g; int id; };
  auto ecmp = [](const E &a, const E &b) { if (a.f != b.f) return a.f > b.f; if (a.g != b.g) return a.g > b.g; return a.id > b.id; };
  std::priority_queue<E, std::vector<E>, decltype(ecmp)> open(ecmp);
  g_nodes.push_back(PNode{s, 0.0, eps == 0 ? 0.0 : heur(s), 0, 1, {}, {}, {}});
  table[s.key()] = 0;
  open.push(E{eps * g_nodes[0].h, 0.0, 0});
  int status = 0, curr = -1, it = 0;
  vec_E<Wp> succ;
  std::vector<decimal_t> cost;
  std::vector<int> act;
  for (;;) {
    for (;;) {  // pop the smallest live entry
      if (open.empty()) { curr = -1; break; }
      const E e = open.top();
      open.pop();
      if (g_nodes[e.id].closed || g_nodes[e.id].g != e.g) continue;
      curr = e.id;
      break;
    }
    if (curr < 0) { status = 1; break; }
    it++;
    g_nodes[curr].closed = 1;
    g_exp.push_back(curr);
    const Wp cw = g_nodes[curr].coord;
    r->env->get_succ(cw, succ, cost, act);
    for (size_t k = 0; k < succ.size(); k++) {
      if (std::isinf(cost[k])) continue;
      Wp tn = succ[k];
      tn.control = cw.control;
      const auto key = tn.key();
      int id;
      auto f = table.find(key);
      if (f == table.end()) {
        id = (int)g_nodes.size();
        g_nodes.push_back(PNode{tn, std::numeric_limits<double>::infinity(), eps == 0 ? 0.0 : heur(tn), 0, 0, {}, {}, {}});
        table[key] = id;
      } else {
        id = f->second;
      }
      g_nodes[id].pred.push_back(curr); g_nodes[id].pact.push_back(act[k]); g_nodes[id].pcost.push_back(cost[k]);
      const double tg = g_nodes[curr].g + cost[k];
      if (tg < g_nodes[id].g) {
        g_nodes[id].g = tg;
        g_nodes[id].closed = 0;
        g_nodes[id].opened = 1;
        open.push(E{tg + eps * g_nodes[id].h, tg, id});
      }
    }
    if (is_goal(g_nodes[curr].coord)) break;
    if (max_expand > 0 && it >= max_expand) { status = 3; break; }
  }
  if (status != 0) return status;
  // recoverTraj: minimise g(pred) + cost, ties -> larger g(pred), then the oldest record
  int node = curr;
  g_traj_nodes.push_back(node);
  while (!g_nodes[node].pred.empty()) {
    int best = -1;
    double min_rhs = std::numeric_limits<double>::infinity(), min_g = std::numeric_limits<double>::infinity();
    for (size_t e = 0; e < g_nodes[node].pred.size(); e++) {
      const double gp = g_nodes[g_nodes[node].pred[e]].g, rhs = gp + g_nodes[node].pcost[e];
      if (min_rhs > rhs) { min_rhs = rhs; min_g = gp; best = (int)e; }
      else if (min_rhs == rhs && min_g < gp) { min_g = gp; best = (int)e; }
    }
    if (best < 0) return 1;
    g_traj_act.push_back(g_nodes[node].pact[best]);
    node = g_nodes[node].pred[best];
    g_traj_nodes.push_back(node);
    if (node == 0) break;
  }
  g_cost = g_nodes[curr].g;
  return 0;
}
int refpoly3_num_expanded() { return (int)g_exp.size(); }
int refpoly3_num_nodes() { return (int)g_nodes.size(); }
double refpoly3_traj_cost() { return g_cost; }
int refpoly3_traj_len() { return (int)g_traj_act.size(); }
void refpoly3_get_expanded(int *ids) { for (size_t i = 0; i < g_exp.size(); i++) ids[i] = g_exp[i]; }
// path in start -> goal order: node ids (len + 1), actions (len)
void refpoly3_get_traj(int *node_ids, int *actions) {
  const size_t n = g_traj_act.size();
  for (size_t i = 0; i <= n && !g_traj_nodes.empty(); i++) node_ids[i] = g_traj_nodes[n - i];
  for (size_t i = 0; i < n; i++) actions[i] = g_traj_act[n - 1 - i];
}
void refpoly3_get_node(int id, double *state, double *g, double *hh) { wp_to(g_nodes[id].coord, state); *g = g_nodes[id].g; *hh = g_nodes[id].h; }
}
