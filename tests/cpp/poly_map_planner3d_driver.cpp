// tests/cpp/poly_map_planner3d_driver.cpp -- MPL::PolyMapPlanner3D as the reference's callers drive a planner (setMap,
// setStartTime, set*Obstacles, the PlannerBase setters, plan, getTraj / getCloseSet / getOpenSet / getExpandedNodes), compiled
// against the reference's poly_map_planner headers with include/mpl_shim ahead of them.  Plans the scene of poly3_scene.h and
// prints one JSON line; a second planner with setLPAstar(true) must refuse.
#include <mpl_external_planner/poly_map_planner/poly_map_planner.h>

#include "poly3_scene.h"

using namespace poly3_scene;

static Polyhedron3D poly(const std::vector<double> &hp) {
  Polyhedron3D P;
  for (size_t i = 0; i + 5 < hp.size(); i += 6) P.add(Hyperplane3D(Vec3f(hp[i], hp[i + 1], hp[i + 2]), Vec3f(hp[i + 3], hp[i + 4], hp[i + 5])));
  return P;
}

int main() {
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

  MPL::PolyMapPlanner3D planner(false);
  planner.setMap(Vec3f(ORI[0], ORI[1], ORI[2]), Vec3f(DIM[0], DIM[1], DIM[2]));
  planner.setStartTime(START_T);
  planner.setStaticObstacles(st);
  planner.setLinearObstacles(lin);
  planner.setNonlinearObstacles(nl);
  planner.setVmax(V_MAX); planner.setAmax(A_MAX); planner.setDt(DT); planner.setU(U); planner.setW(W);
  planner.setEpsilon(EPS); planner.setTol(TOL_POS); planner.setMaxNum(MAX_NUM); planner.setHeurIgnoreDynamics(false);
  Waypoint3D start(Control::ACC), goal(Control::ACC);
  start.pos = Vec3f(START[0], START[1], START[2]);
  start.t = START_T;
  goal.pos = Vec3f(GOAL[0], GOAL[1], GOAL[2]);
  const bool ok = planner.plan(start, goal);
  const auto prs_out = planner.getTraj().getPrimitives();

  MPL::PolyMapPlanner3D lpa(false);  // 3-D LPA*: refused loudly, nothing planned
  lpa.setMap(Vec3f(ORI[0], ORI[1], ORI[2]), Vec3f(DIM[0], DIM[1], DIM[2]));
  lpa.setU(U);
  lpa.setLPAstar(true);
  const bool lpa_ok = lpa.plan(start, goal);
  lpa.updateNodes();
  lpa.getSubStateSpace(1);

  const double cost = planner.getTrajCost();
  printf("{\"planned\": %d, \"status\": %d, \"cost\": %.17g, \"traj_len\": %zu, \"close_set\": %zu, \"open_set\": %zu, \"expanded_nodes\": %zu, \"lpa_planned\": %d, \"prs\": [",
         (int)ok, planner.getResult().status, std::isinf(cost) ? -1.0 : cost, prs_out.size(), planner.getCloseSet().size(), planner.getOpenSet().size(),
         planner.getExpandedNodes().size(), (int)lpa_ok);
  for (size_t i = 0; i < prs_out.size(); i++) {
    printf("%s[", i ? ", " : "");
    for (int ax = 0; ax < 3; ax++)
      for (int k = 0; k < 6; k++) printf("%s%.17g", ax + k ? ", " : "", prs_out[i].pr(ax).coeff()(k));
    printf("]");
  }
  printf("]}\n");
  return 0;
}
