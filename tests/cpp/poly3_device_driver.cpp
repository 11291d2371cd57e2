// tests/cpp/poly3_device_driver.cpp -- plans the scene of poly3_scene.h through the shim's reference-free 3-D plumbing
// (include/mpl_shim/mpl_external_planner/poly_map_planner/poly3_device.h: what PolyMapPlanner<3>::plan() runs) and prints
// the outcome as one JSON line.  Exit code 3: the plumbing failed (no device).
#include <mpl_external_planner/poly_map_planner/poly3_device.h>

#include <cmath>

#include "poly3_scene.h"

using namespace poly3_scene;

int main() {
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
  mplx_shim::Poly3Plan r;
  if (!mplx_shim::poly3_plan(q, r)) return 3;
  int closed = 0;
  for (int32_t c : r.closed) closed += c != 0;
  printf("{\"status\": %d, \"cost\": %.17g, \"n_expanded\": %llu, \"n_nodes\": %llu, \"closed\": %d, \"expanded\": %zu, \"actions\": [", r.res.status, std::isinf(r.res.cost) ? -1.0 : r.res.cost,  // (-1: no trajectory)
         (unsigned long long)r.res.n_expanded, (unsigned long long)r.res.n_nodes, closed, r.expanded.size());
  for (size_t i = 0; i < r.actions.size(); i++) printf("%s%d", i ? ", " : "", r.actions[i]);
  printf("], \"states\": [");
  for (size_t i = 0; i < r.states.size(); i++) printf("%s%.17g", i ? ", " : "", r.states[i]);
  printf("]}\n");
  return 0;
}
