// tests/cpp/poly3_space_driver.cpp -- the five state-space getters of a 3-D moving-obstacle plan on the scene of poly3_scene.h,
// getValidPrimitives / getAllPrimitives included, in one of two builds that print the same JSON line:
//   -DPOLY3_SPACE_WITH_PLANNER  MPL::PolyMapPlanner3D as the reference's callers drive it, compiled against the reference's
//                               poly_map_planner headers with include/mpl_shim ahead of them;
//   (default)                   the reference-free plumbing the planner reads through (poly3_device.h: poly3_plan,
//                               poly3_space_fetch), with Primitive(parent state, U[action], dt) of an ACC state spelled out.
// Planner A plans and answers; planner B plans on the shared device object, after which A's primitives must be refused; planner C
// never plans and must be refused without touching the device.  Exit code 3: the plan did not run (no device).
#ifdef POLY3_SPACE_WITH_PLANNER
#include <mpl_external_planner/poly_map_planner/poly_map_planner.h>
#else
#include <mpl_external_planner/poly_map_planner/poly3_device.h>
#endif

#include <cmath>
#include <cstring>

#include "poly3_scene.h"

using namespace poly3_scene;

typedef std::vector<double> Coeffs;  // 18 per primitive: cx[6], cy[6], cz[6]

// sum over the coefficients of bit pattern x (index + 1), modulo 2^64
static unsigned long long digest(const Coeffs &c) {
  unsigned long long d = 0;
  for (size_t i = 0; i < c.size(); i++) {
    unsigned long long b;
    memcpy(&b, &c[i], 8);
    d += b * (unsigned long long)(i + 1);
  }
  return d;
}
static void print_row(const char *name, const Coeffs &c, size_t first) {
  printf("\"%s\": [", name);
  for (size_t k = 0; k < 18 && first + k < c.size(); k++) printf("%s%.17g", k ? ", " : "", c[first + k]);
  printf("], ");
}

struct Answer {
  int planned = 0, status = -1;
  size_t sizes[5] = {0, 0, 0, 0, 0};  // close set, open set, expanded nodes, valid primitives, all primitives
  Coeffs all;
};

#ifdef POLY3_SPACE_WITH_PLANNER
static Polyhedron3D poly(const std::vector<double> &hp) {
  Polyhedron3D P;
  for (size_t i = 0; i + 5 < hp.size(); i += 6) P.add(Hyperplane3D(Vec3f(hp[i], hp[i + 1], hp[i + 2]), Vec3f(hp[i + 3], hp[i + 4], hp[i + 5])));
  return P;
}
typedef MPL::PolyMapPlanner3D Planner;
static void set_up(Planner &planner) {
  vec_E<VecDf> U;
  const std::vector<double> L = lattice();
  for (size_t i = 0; i < L.size(); i += 3) U.push_back(Vec3f(L[i], L[i + 1], L[i + 2]));
  vec_E<PolyhedronObstacle3D> st;
  st.push_back(PolyhedronObstacle3D(poly(box(0.8)), Vec3f(STATIC_P[0][0], STATIC_P[0][1], STATIC_P[0][2])));
  st.push_back(PolyhedronObstacle3D(poly(octahedron(1.0)), Vec3f(STATIC_P[1][0], STATIC_P[1][1], STATIC_P[1][2])));
  vec_E<PolyhedronLinearObstacle3D> lin;
  PolyhedronLinearObstacle3D lo(poly(box(0.5)), Vec3f(LIN_P[0], LIN_P[1], LIN_P[2]), Vec3f(LIN_V[0], LIN_V[1], LIN_V[2]));
  lo.set_cov_v(LIN_COV);
  lin.push_back(lo);
  vec_E<Primitive3D> prs;
  const std::vector<double> S = nl_segs();
  for (size_t i = 0; i + 18 < S.size(); i += 19) {
    vec_E<Vec6f> cs(3);
    for (int ax = 0; ax < 3; ax++)
      for (int k = 0; k < 6; k++) cs[ax](k) = S[i + 6 * ax + k];
    prs.push_back(Primitive3D(cs, S[i + 18], Control::ACC));
  }
  vec_E<PolyhedronNonlinearObstacle3D> nl;
  PolyhedronNonlinearObstacle3D no(poly(box(0.5)), Trajectory3D(prs), NL_START_T);
  no.disappear_back_ = true;
  nl.push_back(no);
  planner.setMap(Vec3f(ORI[0], ORI[1], ORI[2]), Vec3f(DIM[0], DIM[1], DIM[2]));
  planner.setStartTime(START_T);
  planner.setStaticObstacles(st);
  planner.setLinearObstacles(lin);
  planner.setNonlinearObstacles(nl);
  planner.setVmax(V_MAX); planner.setAmax(A_MAX); planner.setDt(DT); planner.setU(U); planner.setW(W);
  planner.setEpsilon(EPS); planner.setTol(TOL_POS); planner.setMaxNum(MAX_NUM); planner.setHeurIgnoreDynamics(false);
}
static bool plan(Planner &planner, Answer &a) {
  Waypoint3D start(Control::ACC), goal(Control::ACC);
  start.pos = Vec3f(START[0], START[1], START[2]);
  start.t = START_T;
  goal.pos = Vec3f(GOAL[0], GOAL[1], GOAL[2]);
  a.planned = planner.plan(start, goal) ? 1 : 0;
  a.status = planner.getResult().status;
  return planner.getResult().n_nodes > 0;
}
static void ask(const Planner &planner, Answer &a) {
  a.sizes[0] = planner.getCloseSet().size();
  a.sizes[1] = planner.getOpenSet().size();
  a.sizes[2] = planner.getExpandedNodes().size();
  a.sizes[3] = planner.getValidPrimitives().size();
  const auto all = planner.getAllPrimitives();
  a.sizes[4] = all.size();
  a.all.clear();
  for (const auto &pr : all)
    for (int ax = 0; ax < 3; ax++)
      for (int k = 0; k < 6; k++) a.all.push_back(pr.pr(ax).coeff()(k));
}
#else
struct Planner {  // what PolyMapPlanner<3> keeps of its last plan
  mplx_shim::Poly3Plan plan;
  mutable mplx_shim::Poly3Space space;
};
static void set_up(Planner &) {}
static bool plan(Planner &planner, Answer &a) {
  mplx_shim::Poly3Query q;
  q.control = MPLX_ACC;
  q.U = lattice();
  q.dt = DT; q.v_max = V_MAX; q.a_max = A_MAX; q.j_max = J_MAX; q.w = W;
  for (int k = 0; k < 3; k++) { q.ori[k] = ORI[k]; q.dim[k] = DIM[k]; q.start[k] = START[k]; q.goal[k] = GOAL[k]; }
  q.start_t = START_T;
  q.start[12] = START_T;
  for (int i = 0; i < 2; i++) {
    mplx_shim::Poly3Obstacle o;
    o.kind = 0;
    o.hp = i == 0 ? box(0.8) : octahedron(1.0);
    for (int k = 0; k < 3; k++) o.p[k] = STATIC_P[i][k];
    q.obstacles.push_back(o);
  }
  mplx_shim::Poly3Obstacle l;
  l.kind = 1;
  l.hp = box(0.5);
  for (int k = 0; k < 3; k++) { l.p[k] = LIN_P[k]; l.v[k] = LIN_V[k]; }
  l.cov_v = LIN_COV;
  q.obstacles.push_back(l);
  mplx_shim::Poly3Obstacle n;
  n.kind = 2;
  n.hp = box(0.5);
  n.segs = nl_segs();
  n.start_t = NL_START_T;
  n.dis_back = true;
  q.obstacles.push_back(n);
  q.eps = EPS; q.tol_pos = TOL_POS; q.tol_vel = -1; q.max_num = MAX_NUM; q.heur_ignore_dynamics = 0;
  planner.space = mplx_shim::Poly3Space();
  if (!mplx_shim::poly3_plan(q, planner.plan)) return false;
  a.planned = planner.plan.res.status == MPLX_PLAN_OK ? 1 : 0;
  a.status = planner.plan.res.status;
  return planner.plan.res.n_nodes > 0;
}
static size_t primitives(const Planner &planner, bool all, const char *what, Coeffs *out) {
  const mplx_shim::Poly3Space &S = planner.space;
  if (!mplx_shim::poly3_space_fetch(planner.plan.epoch, planner.plan.res, all, planner.space, what)) return 0;
  const std::vector<double> U = lattice();
  size_t n = 0;
  auto add = [&](int32_t parent, int32_t action) {  // Primitive(parent state, U[action], dt) of an ACC state: {0, 0, 0, u, vel, pos} per axis
    n++;
    if (!out) return;
    const double *st = &S.states[(size_t)parent * 13];
    for (int ax = 0; ax < 3; ax++) {
      const double row[6] = {0.0, 0.0, 0.0, U[3 * (size_t)action + (size_t)ax], st[3 + ax], st[ax]};
      out->insert(out->end(), row, row + 6);
    }
  };
  for (size_t i = 0; i < S.parent.size(); i++) add(S.parent[i], S.action[i]);
  if (all)
    for (size_t i = 0; i < S.blocked_parent.size(); i++) add(S.blocked_parent[i], S.blocked_action[i]);
  return n;
}
static void ask(const Planner &planner, Answer &a) {
  for (size_t i = 0; i < planner.plan.closed.size(); i++) {
    a.sizes[0] += planner.plan.closed[i] != 0;
    a.sizes[1] += planner.plan.opened[i] != 0 && planner.plan.closed[i] == 0;
  }
  a.sizes[2] = planner.plan.expanded.size();
  a.sizes[3] = primitives(planner, false, "getValidPrimitives()", nullptr);
  a.all.clear();
  a.sizes[4] = primitives(planner, true, "getAllPrimitives()", &a.all);
}
#endif

int main() {
  Planner never;  // (asked first: nothing has touched the device yet)
  Answer n;
  ask(never, n);
  Planner first, other;
  set_up(first);
  set_up(other);
  Answer a, b, after;
  const bool ran = plan(first, a);
  if (ran) ask(first, a);
  if (ran && plan(other, b)) ask(first, after);  // the shared device object now holds the other planner's plan
  printf("{\"planned\": %d, \"status\": %d, \"sizes\": [%zu, %zu, %zu, %zu, %zu], ", a.planned, a.status, a.sizes[0], a.sizes[1], a.sizes[2], a.sizes[3], a.sizes[4]);
  print_row("first", a.all, 0);
  print_row("last", a.all, a.all.size() >= 18 ? a.all.size() - 18 : 0);
  printf("\"digest\": \"%llu\", \"other_planned\": %d, \"after_other\": [%zu, %zu], \"never\": [%zu, %zu]}\n", digest(a.all), b.planned, after.sizes[3], after.sizes[4],
         n.sizes[3], n.sizes[4]);
  return ran ? 0 : 3;
}
