// tests/cpp/poly_map_getters_driver.cpp -- the five state-space getters of MPL::PolyMapPlanner2D (getCloseSet, getOpenSet,
// getExpandedNodes, getValidPrimitives, getAllPrimitives) as poly_map_planner_node.cpp:105-124 and
// poly_map_replanner_node.cpp:156-158,184,234 call them, compiled against the reference's poly_map_planner headers with
// include/mpl_shim ahead of them: in A* mode, with setLPAstar(true), through a PlannerBase pointer, after another planner has
// planned on the shared device object, and on a 3-D planner (primitives refused).  The world is the replanner flow's five
// moving boxes (tests/cpp/poly2_space_driver.cpp).  Prints one JSON line; without a GPU the planners refuse and every set is empty.
#include <mpl_external_planner/poly_map_planner/poly_map_planner.h>

#include <string>

static Polyhedron2D rect(double h) {
  Polyhedron2D P;
  P.add(Hyperplane2D(Vec2f(-h, 0), Vec2f(-1, -0.0)));
  P.add(Hyperplane2D(Vec2f(h, 0), Vec2f(1, 0)));
  P.add(Hyperplane2D(Vec2f(0, -h), Vec2f(-0.0, -1)));
  P.add(Hyperplane2D(Vec2f(0, h), Vec2f(0, 1)));
  return P;
}

template <class Planner>
static void setup(Planner &pl, const vec_E<VecDf> &U, bool lpa) {
  const double OBS[5][4] = {{6, 12, 0, -0.6}, {10, 6, 0, 0.5}, {13, 14, -0.3, -0.7}, {16, 9, 0, 0.4}, {8, 9.5, 0.4, 0.0}};
  pl.setMap(Vec2f(0, 0), Vec2f(20, 20));
  pl.setStartTime(0.0);
  vec_E<PolyhedronLinearObstacle2D> lin;
  for (int k = 0; k < 5; k++) {
    PolyhedronLinearObstacle2D o(rect(1.0), Vec2f(OBS[k][0], OBS[k][1]), Vec2f(OBS[k][2], OBS[k][3]));
    o.set_cov_v(0.2);
    lin.push_back(o);
  }
  pl.setLinearObstacles(lin);
  pl.setVmax(2.0); pl.setAmax(1.0); pl.setDt(1.0); pl.setU(U); pl.setW(10.0);
  pl.setEpsilon(1.0); pl.setTol(0.5); pl.setMaxNum(2000); pl.setHeurIgnoreDynamics(true);
  pl.setLPAstar(lpa);
}

static std::string json;  // (printed whole at the end: the planners print their refusals in between)
template <class Base>
static void sizes(const char *name, const Base &pl) {
  char buf[256];
  snprintf(buf, sizeof(buf), "\"%s\": [%zu, %zu, %zu, %zu, %zu], ", name, pl.getCloseSet().size(), pl.getOpenSet().size(), pl.getExpandedNodes().size(),
           pl.getValidPrimitives().size(), pl.getAllPrimitives().size());
  json += buf;
}

int main() {
  vec_E<VecDf> U;
  for (int dx = -1; dx <= 1; dx++)
    for (int dy = -1; dy <= 1; dy++) U.push_back(Vec2f(dx, dy));
  Waypoint2D start(Control::ACC), goal(Control::ACC);
  start.pos = Vec2f(0.5, 10);
  goal.pos = Vec2f(19, 10);

  MPL::PolyMapPlanner2D astar(false), lpa(false), fresh(false);
  setup(astar, U, false);
  setup(lpa, U, true);
  setup(fresh, U, false);
  sizes("before_plan", fresh);  // no plan yet: empty, silently (as upstream before plan())
  const bool ok_a = astar.plan(start, goal);
  sizes("astar", astar);
  const MPL::PlannerBase<2, Waypoint2D> &base = astar;  // through a base pointer: the planner's own getters
  sizes("astar_base", base);
  const bool ok_l = lpa.plan(start, goal);  // (its own handle: the A* planner's space on the shared object is still there)
  sizes("lpa", lpa);
  sizes("astar_after_lpa", astar);
  Waypoint2D start2 = start;
  start2.pos = Vec2f(0.5, 4);
  const bool ok_f = fresh.plan(start2, goal);  // another A* planner on the shared device object
  sizes("other", fresh);
  sizes("astar_after_other", astar);  // refused: empty

  MPL::PolyMapPlanner3D p3(false);
  const size_t v3 = p3.getValidPrimitives().size(), a3 = p3.getAllPrimitives().size();
  printf("{%s\"planned\": [%d, %d, %d], \"valid3\": %zu, \"all3\": %zu}\n", json.c_str(), (int)ok_a, (int)ok_l, (int)ok_f, v3, a3);
  return 0;
}
