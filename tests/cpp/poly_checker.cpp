// tests/cpp/poly_checker.cpp -- CPU checker of the moving-obstacle environment at any dimension (Dim = 2 and 3), compiled with
// g++ at test time and loaded through ctypes (tests/poly_checker.py).  TEST INFRASTRUCTURE ONLY.
//
// Restates, in its own words and templated on Dim, what the reference's in-tree environment computes (paths relative to the
// reference repo):
//   mpl_external_planner/include/mpl_external_planner/poly_map_planner/env_poly_map.h:45-73   get_succ, intrinsic cost
//   .../poly_map_planner/poly_map_util.h:39-109                      setBoundingBox (2-D and 3-D), isInside, isFree(pt, t), isFree(pr, t)
//   .../poly_map_planner/primitive_geometry_utils.h:5-173            collide() x 3 (static / linear / nonlinear obstacle)
//   .../poly_map_planner/simple_obstacle.h:6-166                     obstacle classes (inside, poly(t))
// on the very basis classes the compiled reference (oracle/_ref/libpolymap_ref.so) is built against: include/mpl_shim's
// Primitive / Trajectory / Waypoint, solve() and Polyhedron.  Every floating-point expression keeps the reference's operands
// and order (n.dot(x) is s = 0, s += n(i) x(i) over i < Dim; vector sums left to right), -ffp-contract=off, so at Dim = 2 it
// agrees with libpolymap_ref bit for bit (the tests pin that) and at Dim = 3 it is what the reference's templates compute.
//
// The best-first search is the one of refpoly_plan (oracle/ref_stubs/poly_map_ref_api.cpp): OPEN ordered by (f, g, id),
// blocked successors not materialised, re-open on improvement, goal test after the expansion, recoverTraj minimising
// g(pred) + cost with ties to the larger g(pred), then the oldest record.  The dynamics-aware heuristic goes through the CPU
// oracle's orc_heuristic (handed over as a function pointer), the distance heuristic is w |dp|_inf / v_max.  Goal test:
// |dp|_inf <= tol_pos and, with tol_vel >= 0, |dv|_inf <= tol_vel (refpoly_plan has position only: the 2-D anchor uses tol_vel < 0).
#include <decomp_geometry/polyhedron.h>
#include <mpl_basis/math.h>
#include <mpl_basis/trajectory.h>

#include <cmath>
#include <limits>
#include <map>
#include <queue>
#include <vector>

namespace {

const double INF = std::numeric_limits<double>::infinity();

template <int Dim>
struct Obstacle {
  int kind = 0;  // 0 static, 1 linear, 2 nonlinear
  Polyhedron<Dim> shape;
  Vecf<Dim> p, v;
  double cov_v = 0, start_t = 0;
  Trajectory<Dim> traj;
  bool dis_front = false, dis_back = false;
};

// n.dot(x) of the shim's vector: s = 0, then s += n(i) * x(i) in axis order
template <int Dim>
double dot(const Vecf<Dim> &n, const Vecf<Dim> &x) {
  double s = 0.0;
  for (int i = 0; i < Dim; i++) s += n(i) * x(i);
  return s;
}
template <int Dim>
bool in_poly(const Polyhedron<Dim> &poly, const Vecf<Dim> &pt) {  // Polyhedron::inside
  for (const auto &h : poly.vs_) {
    Vecf<Dim> d;
    for (int i = 0; i < Dim; i++) d(i) = pt(i) - h.p_(i);
    if (dot<Dim>(h.n_, d) > 1e-10) return false;
  }
  return true;
}

template <int Dim>
struct Env {
  Polyhedron<Dim> bbox;
  double start_t = 0;
  std::vector<Obstacle<Dim>> st, lin, nl;
  vec_E<VecDf> U;
  double dt = 1, v_max = -1, a_max = -1, j_max = -1, w = 10;

  // ---- obstacle classes
  static bool inside_at(const Obstacle<Dim> &o, const Vecf<Dim> &pt, const Vecf<Dim> &at) {
    Vecf<Dim> d;
    for (int i = 0; i < Dim; i++) d(i) = pt(i) - at(i);
    return in_poly<Dim>(o.shape, d);
  }
  static bool inside_linear(const Obstacle<Dim> &o, const Vecf<Dim> &pt, double t) {
    Polyhedron<Dim> moved = o.shape;  // poly(t): each point moves by (v t + p) + (cov_v n) t
    for (auto &h : moved.vs_)
      for (int i = 0; i < Dim; i++) h.p_(i) = h.p_(i) + ((o.v(i) * t + o.p(i)) + (h.n_(i) * o.cov_v) * t);
    return in_poly<Dim>(moved, pt);
  }
  static bool present(const Obstacle<Dim> &o, double tt) {
    const double T = o.traj.getTotalTime();
    return (tt <= T && tt >= 0) || (tt < 0 && !o.dis_front) || (tt > T && !o.dis_back);
  }
  static bool inside_nonlinear(const Obstacle<Dim> &o, const Vecf<Dim> &pt, double t) {
    const double tt = t + o.start_t;
    const Waypoint<Dim> wq = o.traj.evaluate(tt);
    return present(o, tt) && inside_at(o, pt, wq.pos);
  }

  // ---- the three collide()
  static void coeffs(const Primitive<Dim> &pr, std::vector<Vec6f> &cs) {
    cs.resize(Dim);
    for (int i = 0; i < Dim; i++) cs[i] = pr.pr(i).coeff();
  }
  static bool collide_static(const Primitive<Dim> &pr, const Obstacle<Dim> &o, const Vecf<Dim> &at) {
    std::vector<Vec6f> cs;
    coeffs(pr, cs);
    for (const auto &h : o.shape.vs_) {
      double k[6] = {0, 0, 0, 0, 0, 0};
      for (int i = 0; i < Dim; i++)
        for (int m = 0; m < 6; m++) k[m] += h.n_(i) * cs[i](m);
      k[0] /= 120.0; k[1] /= 24.0; k[2] /= 6.0; k[3] /= 2.0; k[4] /= 1.0;
      Vecf<Dim> q;
      for (int i = 0; i < Dim; i++) q(i) = h.p_(i) + at(i);
      k[5] -= dot<Dim>(h.n_, q);
      for (double r : solve(k[0], k[1], k[2], k[3], k[4], k[5]))
        if (r >= 0 && r <= pr.t() && inside_at(o, pr.evaluate(r).pos, at)) return true;
    }
    return false;
  }
  static bool collide_linear(const Primitive<Dim> &pr, const Obstacle<Dim> &o, double t) {
    std::vector<Vec6f> cs;
    coeffs(pr, cs);
    for (const auto &h : o.shape.vs_) {
      Vecf<Dim> cv;
      for (int i = 0; i < Dim; i++) cv(i) = o.v(i) + h.n_(i) * o.cov_v;
      double k[6] = {0, 0, 0, 0, 0, 0};
      for (int i = 0; i < Dim; i++)
        for (int m = 0; m < 6; m++) k[m] += h.n_(i) * cs[i](m);
      k[0] /= 120.0; k[1] /= 24.0; k[2] /= 6.0; k[3] /= 2.0;
      k[4] -= dot<Dim>(h.n_, cv);
      Vecf<Dim> q;
      for (int i = 0; i < Dim; i++) q(i) = (h.p_(i) + o.p(i)) + cv(i) * t;
      k[5] -= dot<Dim>(h.n_, q);
      for (double r : solve(k[0], k[1], k[2], k[3], k[4], k[5]))
        if (r >= 0 && r <= pr.t() && inside_linear(o, pr.evaluate(r).pos, r + t)) return true;
    }
    return false;
  }
  static bool collide_nonlinear(const Primitive<Dim> &pr, const Obstacle<Dim> &o, double t) {
    std::vector<Vec6f> cs;
    coeffs(pr, cs);
    const double tt = t + o.start_t;
    const auto segs = o.traj.getPrimitives();
    int first = -1;
    double T0 = 0.0;  // start time of the segment under consideration
    for (size_t i = 0; i < segs.size(); i++) {
      if (tt >= T0 && tt < T0 + segs[i].t()) { first = (int)i; break; }
      T0 += segs[i].t();
    }
    if (first < 0) return present(o, tt) && collide_static(pr, o, o.traj.evaluate(tt).pos);
    for (size_t id = (size_t)first; id < segs.size(); id++) {
      const double resid = T0 - tt < 0 ? 0 : T0 - tt;
      const double from = resid <= 0 ? tt : T0;
      if (resid > pr.t()) break;
      const Waypoint<Dim> ws = o.traj.evaluate(from);
      for (const auto &h : o.shape.vs_) {
        double k[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < Dim; i++) {
          k[0] += h.n_(i) * cs[i](0);
          k[1] += h.n_(i) * cs[i](1);
          k[2] += h.n_(i) * cs[i](2) - h.n_(i) * ws.jrk(i);
          k[3] += h.n_(i) * cs[i](3) - h.n_(i) * ws.acc(i);
          k[4] += h.n_(i) * cs[i](4) - h.n_(i) * ws.vel(i);
          k[5] += h.n_(i) * cs[i](5) - h.n_(i) * (h.p_(i) + ws.pos(i));
        }
        k[0] /= 120; k[1] /= 24; k[2] /= 6; k[3] /= 2;
        for (double r : solve(k[0], k[1], k[2], k[3], k[4], k[5]))
          if (r >= resid && r <= pr.t() && T0 + segs[id].t() >= r + from && T0 <= r + from && inside_nonlinear(o, pr.evaluate(r).pos, r + t)) return true;
      }
      T0 += segs[id].t();
    }
    return false;
  }

  // ---- PolyMapUtil
  bool is_inside(const Vecf<Dim> &pt) const { return in_poly<Dim>(bbox, pt); }
  bool is_free(const Vecf<Dim> &pt, double t) const {
    for (const auto &o : st)
      if (inside_at(o, pt, o.p)) return false;
    for (const auto &o : lin)
      if (inside_linear(o, pt, t - start_t)) return false;
    for (const auto &o : nl)
      if (inside_nonlinear(o, pt, t - start_t)) return false;
    return true;
  }
  bool is_free(const Primitive<Dim> &pr, double t) const {
    if (!is_free(pr.evaluate(0).pos, t)) return false;
    for (const auto &o : st)
      if (collide_static(pr, o, o.p)) return false;
    for (const auto &o : lin)
      if (collide_linear(pr, o, t - start_t)) return false;
    for (const auto &o : nl)
      if (collide_nonlinear(pr, o, t - start_t)) return false;
    return true;
  }
  // ---- env_poly_map
  double cost(const Primitive<Dim> &pr) const { return pr.J(pr.control()) + 0.001 * pr.J(Control::VEL) + w * dt; }
  void get_succ(const Waypoint<Dim> &curr, vec_E<Waypoint<Dim>> &succ, std::vector<double> &succ_cost, std::vector<int> &act) const {
    succ.clear(); succ_cost.clear(); act.clear();
    for (size_t i = 0; i < U.size(); i++) {
      const Primitive<Dim> pr(curr, U[i], dt);
      Waypoint<Dim> tn = pr.evaluate(dt);
      if (!is_inside(tn.pos) || !validate_primitive(pr, v_max, a_max, j_max)) continue;
      succ_cost.push_back(is_free(pr, curr.t) ? cost(pr) : INF);
      tn.t = curr.t + dt;
      tn.enable_t = true;
      succ.push_back(tn);
      act.push_back((int)i);
    }
  }
};

// PolyMapUtil::setBoundingBox: the faces in the reference's order, normals -e_k then +e_k
void set_box(Env<2> &E, const double *o, const double *d) {
  Polyhedron<2> B;
  B.add(Hyperplane<2>(Vec2f(o[0] + 0.0, o[1] + d[1] / 2), Vec2f(-1.0, -0.0)));
  B.add(Hyperplane<2>(Vec2f(o[0] + d[0] / 2, o[1] + 0.0), Vec2f(-0.0, -1.0)));
  B.add(Hyperplane<2>(Vec2f((o[0] + d[0]) - 0.0, (o[1] + d[1]) - d[1] / 2), Vec2f(1.0, 0.0)));
  B.add(Hyperplane<2>(Vec2f((o[0] + d[0]) - d[0] / 2, (o[1] + d[1]) - 0.0), Vec2f(0.0, 1.0)));
  E.bbox = B;
}
void set_box(Env<3> &E, const double *o, const double *d) {
  Polyhedron<3> B;
  const double h0 = d[0] / 2, h1 = d[1] / 2, h2 = d[2] / 2;
  B.add(Hyperplane<3>(Vec3f(o[0] + 0.0, o[1] + h1, o[2] + h2), Vec3f(-1.0, -0.0, -0.0)));
  B.add(Hyperplane<3>(Vec3f(o[0] + h0, o[1] + 0.0, o[2] + h2), Vec3f(-0.0, -1.0, -0.0)));
  B.add(Hyperplane<3>(Vec3f(o[0] + h0, o[1] + h2, o[2] + 0.0), Vec3f(-0.0, -0.0, -1.0)));  // (the reference's dim(2) / 2 on the y axis)
  B.add(Hyperplane<3>(Vec3f((o[0] + d[0]) - 0.0, (o[1] + d[1]) - h1, (o[2] + d[2]) - h2), Vec3f(1.0, 0.0, 0.0)));
  B.add(Hyperplane<3>(Vec3f((o[0] + d[0]) - h0, (o[1] + d[1]) - 0.0, (o[2] + d[2]) - h2), Vec3f(0.0, 1.0, 0.0)));
  B.add(Hyperplane<3>(Vec3f((o[0] + d[0]) - h0, (o[1] + d[1]) - h1, (o[2] + d[2]) - 0.0), Vec3f(0.0, 0.0, 1.0)));
  E.bbox = B;
}

// layout of orc_waypoint (oracle/mpl_oracle.h)
struct OrcWaypoint { double pos[3], vel[3], acc[3], jrk[3]; double yaw, t; int32_t control, enable_t; };
typedef double (*orc_heur_fn)(const void *planner, const void *waypoint);
orc_heur_fn g_heur_fn = nullptr;
const void *g_heur_planner = nullptr;

struct Base {
  virtual ~Base() {}
  virtual void add(int kind, int n_hp, const double *hp, const double *p, const double *v, double cov_v, int n_seg, const double *segs, int control, double start_t, int df, int db) = 0;
  virtual void set_env(int n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) = 0;
  virtual int get_succ(const double *state, int control, double *succ, double *cost, int *action) = 0;
  virtual bool is_inside(const double *pt) const = 0;
  virtual bool is_free_point(const double *pt, double t) const = 0;
  virtual int plan(const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) = 0;
  // results of the last plan
  std::vector<int> expanded, traj_nodes, traj_act;
  double traj_cost = INF;
  virtual int num_nodes() const = 0;
  virtual void node(int id, double *state, double *g, double *h, int *closed, int *opened) const = 0;
};

template <int Dim>
struct Checker : Base {
  Env<Dim> E;
  struct Node { Waypoint<Dim> coord; double g, h; int closed, opened; std::vector<int> pred, pact; std::vector<double> pcost; };
  std::vector<Node> nodes;

  static Waypoint<Dim> from(const double *s, int control) {  // pos vel acc jrk (Dim each) t
    Waypoint<Dim> w((Control::Control)control);
    for (int i = 0; i < Dim; i++) { w.pos(i) = s[i]; w.vel(i) = s[Dim + i]; w.acc(i) = s[2 * Dim + i]; w.jrk(i) = s[3 * Dim + i]; }
    w.t = s[4 * Dim];
    return w;
  }
  static void to(const Waypoint<Dim> &w, double *s) {
    for (int i = 0; i < Dim; i++) { s[i] = w.pos(i); s[Dim + i] = w.vel(i); s[2 * Dim + i] = w.acc(i); s[3 * Dim + i] = w.jrk(i); }
    s[4 * Dim] = w.t;
  }
  static Polyhedron<Dim> shape(int n_hp, const double *hp) {
    Polyhedron<Dim> P;
    for (int k = 0; k < n_hp; k++) {
      Vecf<Dim> p, n;
      for (int i = 0; i < Dim; i++) { p(i) = hp[2 * Dim * k + i]; n(i) = hp[2 * Dim * k + Dim + i]; }
      P.add(Hyperplane<Dim>(p, n));
    }
    return P;
  }
  void add(int kind, int n_hp, const double *hp, const double *p, const double *v, double cov_v, int n_seg, const double *segs, int control, double start_t, int df,
           int db) override {
    Obstacle<Dim> o;
    o.kind = kind;
    o.shape = shape(n_hp, hp);
    for (int i = 0; i < Dim; i++) { o.p(i) = p ? p[i] : 0.0; o.v(i) = v ? v[i] : 0.0; }
    o.cov_v = cov_v;
    if (kind == 2) {
      vec_E<Primitive<Dim>> prs;
      for (int k = 0; k < n_seg; k++) {
        vec_E<Vec6f> cs(Dim);
        for (int i = 0; i < Dim; i++)
          for (int m = 0; m < 6; m++) cs[i](m) = segs[(6 * Dim + 1) * k + 6 * i + m];
        prs.push_back(Primitive<Dim>(cs, segs[(6 * Dim + 1) * k + 6 * Dim], (Control::Control)control));
      }
      o.traj = Trajectory<Dim>(prs);
      o.start_t = start_t;
      o.dis_front = df != 0;
      o.dis_back = db != 0;
      E.nl.push_back(o);
    } else {
      (kind == 0 ? E.st : E.lin).push_back(o);
    }
  }
  void set_env(int n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) override {
    E.U.clear();
    for (int k = 0; k < n_u; k++) {
      Vecf<Dim> u;
      for (int i = 0; i < Dim; i++) u(i) = U[Dim * k + i];
      E.U.push_back(u);
    }
    E.dt = dt; E.v_max = v_max; E.a_max = a_max; E.j_max = j_max; E.w = w;
  }
  int get_succ(const double *state, int control, double *succ, double *cost, int *action) override {
    vec_E<Waypoint<Dim>> s;
    std::vector<double> c;
    std::vector<int> a;
    E.get_succ(from(state, control), s, c, a);
    for (size_t i = 0; i < s.size(); i++) { to(s[i], succ + (4 * Dim + 1) * i); cost[i] = c[i]; action[i] = a[i]; }
    return (int)s.size();
  }
  static Vecf<Dim> point(const double *x) {
    Vecf<Dim> p;
    for (int i = 0; i < Dim; i++) p(i) = x[i];
    return p;
  }
  bool is_inside(const double *pt) const override { return E.is_inside(point(pt)); }
  bool is_free_point(const double *pt, double t) const override { return E.is_free(point(pt), t); }
  double linf(const Waypoint<Dim> &x, const Waypoint<Dim> &g) const {
    double d = 0;
    for (int i = 0; i < Dim; i++) d = std::max(d, std::fabs(x.pos(i) - g.pos(i)));
    return d;
  }
  int plan(const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) override {
    nodes.clear(); expanded.clear(); traj_nodes.clear(); traj_act.clear();
    traj_cost = INF;
    Waypoint<Dim> s = from(start, control), g = from(goal, control);
    s.enable_t = true;
    if (!E.is_inside(s.pos)) return 2;  // PlannerBase::plan: ENV_->is_free(start.pos)
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
      const double d = linf(x, g);
      return E.v_max > 0 ? E.w * d / E.v_max : E.w * d;
    };
    auto is_goal = [&](const Waypoint<Dim> &x) {  // position within tol_pos; a goal with a velocity and tol_vel >= 0: velocity too
      bool ok = linf(x, g) <= tol_pos;
      if (ok && (control & 2) && tol_vel >= 0) {
        double d = 0;
        for (int i = 0; i < Dim; i++) d = std::max(d, std::fabs(x.vel(i) - g.vel(i)));
        ok = d <= tol_vel;
      }
      return ok;
    };
    if (is_goal(s)) { traj_cost = 0; return 0; }
    std::map<std::vector<int>, int> table;
    struct Entry { double f, g; int id; };
    auto later = [](const Entry &a, const Entry &b) { if (a.f != b.f) return a.f > b.f; if (a.g != b.g) return a.g > b.g; return a.id > b.id; };
    std::priority_queue<Entry, std::vector<Entry>, decltype(later)> open(later);
    nodes.push_back(Node{s, 0.0, heur(s), 0, 1, {}, {}, {}});
    table[s.key()] = 0;
    open.push(Entry{eps * nodes[0].h, 0.0, 0});
    int status = 0, curr = -1, it = 0;
    vec_E<Waypoint<Dim>> succ;
    std::vector<double> cost;
    std::vector<int> act;
    for (;;) {
      curr = -1;
      while (!open.empty()) {  // lazy deletion: a stale entry is skipped
        const Entry e = open.top();
        open.pop();
        if (nodes[e.id].closed || nodes[e.id].g != e.g) continue;
        curr = e.id;
        break;
      }
      if (curr < 0) { status = 1; break; }
      it++;
      nodes[curr].closed = 1;
      expanded.push_back(curr);
      const Waypoint<Dim> cw = nodes[curr].coord;
      E.get_succ(cw, succ, cost, act);
      for (size_t k = 0; k < succ.size(); k++) {
        if (std::isinf(cost[k])) continue;
        Waypoint<Dim> tn = succ[k];
        tn.control = cw.control;
        const auto key = tn.key();
        auto f = table.find(key);
        int id;
        if (f == table.end()) {
          id = (int)nodes.size();
          nodes.push_back(Node{tn, INF, heur(tn), 0, 0, {}, {}, {}});
          table[key] = id;
        } else {
          id = f->second;
        }
        nodes[id].pred.push_back(curr); nodes[id].pact.push_back(act[k]); nodes[id].pcost.push_back(cost[k]);
        const double tg = nodes[curr].g + cost[k];
        if (tg < nodes[id].g) {
          nodes[id].g = tg;
          nodes[id].closed = 0;
          nodes[id].opened = 1;
          open.push(Entry{tg + eps * nodes[id].h, tg, id});
        }
      }
      if (is_goal(nodes[curr].coord)) break;
      if (max_expand > 0 && it >= max_expand) { status = 3; break; }
    }
    if (status != 0) return status;
    int node = curr;
    traj_nodes.push_back(node);
    while (!nodes[node].pred.empty()) {
      int best = -1;
      double min_rhs = INF, min_g = INF;
      for (size_t e = 0; e < nodes[node].pred.size(); e++) {
        const double gp = nodes[nodes[node].pred[e]].g, rhs = gp + nodes[node].pcost[e];
        if (min_rhs > rhs) { min_rhs = rhs; min_g = gp; best = (int)e; }
        else if (min_rhs == rhs && min_g < gp) { min_g = gp; best = (int)e; }
      }
      if (best < 0) return 1;
      traj_act.push_back(nodes[node].pact[best]);
      node = nodes[node].pred[best];
      traj_nodes.push_back(node);
      if (node == 0) break;
    }
    traj_cost = nodes[curr].g;
    return 0;
  }
  int num_nodes() const override { return (int)nodes.size(); }
  void node(int id, double *state, double *g, double *h, int *closed, int *opened) const override {
    to(nodes[id].coord, state);
    *g = nodes[id].g; *h = nodes[id].h; *closed = nodes[id].closed; *opened = nodes[id].opened;
  }
};

}  // namespace

extern "C" {
// ori / dim: Dim doubles each
void *pc_create(int dim, const double *ori, const double *size, double start_t) {
  Base *b = nullptr;
  if (dim == 2) { auto *c = new Checker<2>(); set_box(c->E, ori, size); c->E.start_t = start_t; b = c; }
  if (dim == 3) { auto *c = new Checker<3>(); set_box(c->E, ori, size); c->E.start_t = start_t; b = c; }
  return b;
}
void pc_destroy(void *h) { delete (Base *)h; }
// hp: n_hp x {p[Dim], n[Dim]}; segs: n_seg x {c[Dim][6], T}
void pc_add_static(void *h, int n_hp, const double *hp, const double *p) { ((Base *)h)->add(0, n_hp, hp, p, nullptr, 0.0, 0, nullptr, 0, 0.0, 0, 0); }
void pc_add_linear(void *h, int n_hp, const double *hp, const double *p, const double *v, double cov_v) { ((Base *)h)->add(1, n_hp, hp, p, v, cov_v, 0, nullptr, 0, 0.0, 0, 0); }
void pc_add_nonlinear(void *h, int n_hp, const double *hp, int n_seg, const double *segs, int control, double start_t, int df, int db) {
  ((Base *)h)->add(2, n_hp, hp, nullptr, nullptr, 0.0, n_seg, segs, control, start_t, df, db);
}
void pc_set_env(void *h, int n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) { ((Base *)h)->set_env(n_u, U, dt, v_max, a_max, j_max, w); }
// state: pos vel acc jrk (Dim each) t; succ: n_u x (4 Dim + 1); returns the number emitted
int pc_get_succ(void *h, const double *state, int control, double *succ, double *cost, int *action) { return ((Base *)h)->get_succ(state, control, succ, cost, action); }
// PolyMapUtil::isInside(pt) and isFree(pt, t); pt: Dim doubles
int pc_is_inside(void *h, const double *pt) { return ((Base *)h)->is_inside(pt) ? 1 : 0; }
int pc_is_free_point(void *h, const double *pt, double t) { return ((Base *)h)->is_free_point(pt, t) ? 1 : 0; }
void pc_set_heuristic(void *fn, const void *planner) { g_heur_fn = (orc_heur_fn)fn; g_heur_planner = planner; }
int pc_plan(void *h, const double *start, const double *goal, int control, double eps, double tol_pos, double tol_vel, int max_expand, int heur_mode) {
  return ((Base *)h)->plan(start, goal, control, eps, tol_pos, tol_vel, max_expand, heur_mode);
}
int pc_num_expanded(void *h) { return (int)((Base *)h)->expanded.size(); }
int pc_num_nodes(void *h) { return ((Base *)h)->num_nodes(); }
double pc_traj_cost(void *h) { return ((Base *)h)->traj_cost; }
int pc_traj_len(void *h) { return (int)((Base *)h)->traj_act.size(); }
void pc_get_expanded(void *h, int *ids) {
  const Base *b = (Base *)h;
  for (size_t i = 0; i < b->expanded.size(); i++) ids[i] = b->expanded[i];
}
// path in start -> goal order: node ids (len + 1), actions (len)
void pc_get_traj(void *h, int *node_ids, int *actions) {
  const Base *b = (Base *)h;
  const size_t n = b->traj_act.size();
  for (size_t i = 0; i <= n && !b->traj_nodes.empty(); i++) node_ids[i] = b->traj_nodes[n - i];
  for (size_t i = 0; i < n; i++) actions[i] = b->traj_act[n - 1 - i];
}
void pc_get_node(void *h, int id, double *state, double *g, double *hh, int *closed, int *opened) { ((Base *)h)->node(id, state, g, hh, closed, opened); }
}
