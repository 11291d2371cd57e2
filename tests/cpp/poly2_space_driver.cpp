// poly2_space_driver.cpp -- the state space of a 2-D moving-obstacle plan read through include/mpl_shim's reference-free
// poly2_space.h, exactly as MPL::PolyMapPlanner<2>'s getters read it, on a scene hard-coded here and, identically, in
// tests/test_poly_space_shim.py (five 2 m boxes moving at constant velocity in a 20 m square: the replanner flow's world).
//   (no argument)  A* mode: plan on a device object, fetch, print the sets; then a second plan on the same object (another
//                  planner's) and the first planner's fetch again: refused, empty
//   lpa            setLPAstar(true) mode: three ticks of the replanner flow on an mplx_plpa handle; after each plan the sizes
//                  the five getters would have, next to the counts taken from the mplx_plpa_result_* entries directly
// Prints one JSON object on its last line.  Exit code 3: no HIP device.
#include <mpl_external_planner/poly_map_planner/poly2_space.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
const double OBS[5][4] = {{6, 12, 0, -0.6}, {10, 6, 0, 0.5}, {13, 14, -0.3, -0.7}, {16, 9, 0, 0.4}, {8, 9.5, 0.4, 0.0}};  // p, v
const double RECT[16] = {-1, 0, -1, -0.0, 1, 0, 1, 0, 0, -1, -0.0, -1, 0, 1, 0, 1};
const double DT = 1.0, V_MAX = 2.0, A_MAX = 1.0, J_MAX = -1.0, W = 10.0, EPS = 1.0, TOL_POS = 0.5;
const int MAX_EXPAND = 2000;

bool ok(mplx_poly *p, int rc) {
  if (rc == MPLX_OK) return true;
  printf("error: %s\n", mplx_poly_last_error(p));
  return false;
}
// the world as it is at time t (poly_map_replanner_node.cpp: setLinearObstacles(obstacles at t) + setStartTime(t))
bool world_at(mplx_poly *p, double t) {
  const double ori[2] = {0, 0}, dim[2] = {20, 20};
  if (!ok(p, mplx_poly_begin(p, 1)) || !ok(p, mplx_poly_set_world(p, 0, ori, dim, t))) return false;
  for (int k = 0; k < 5; k++) {
    const double v[2] = {OBS[k][2], OBS[k][3]}, pt[2] = {OBS[k][0] + v[0] * t, OBS[k][1] + v[1] * t};
    if (!ok(p, mplx_poly_add_linear(p, 0, 4, RECT, pt, v, 0.2))) return false;
  }
  return ok(p, mplx_poly_commit(p));
}
bool setup(mplx_poly *p) {
  std::vector<double> U;
  for (int dx = -1; dx <= 1; dx++)
    for (int dy = -1; dy <= 1; dy++) { U.push_back(dx); U.push_back(dy); }
  return ok(p, mplx_poly_config(p, MPLX_ACC, 9, U.data(), DT, V_MAX, A_MAX, J_MAX, W));
}
void print_array(const char *name, const std::vector<double> &v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%.17g", i ? ", " : "", v[i]);
  printf("]");
}

int run_astar(mplx_poly *p) {
  double start[9] = {0.5, 10, 0, 0, 0, 0, 0, 0, 0}, goal[9] = {19, 10, 0, 0, 0, 0, 0, 0, 0};
  const int32_t world = 0;
  mplx_result res = mplx_result();
  if (!setup(p) || !world_at(p, 0.0) || !ok(p, mplx_poly_set_record(p, 1u << 20)) || !ok(p, mplx_poly_set_capacity(p, 1, 1u << 20, 1u << 22, 1u << 21))) return 1;
  if (!ok(p, mplx_poly_plan_batch(p, 1, &world, start, goal, EPS, TOL_POS, -1.0, MAX_EXPAND, 1, &res))) return 1;
  const uint64_t epoch = mplx_poly_plan_epoch(p);
  mplx_shim::Poly2Space sp;
  if (!mplx_shim::poly2_space_fetch(p, 0, epoch, res, false, sp, "getCloseSet()")) return 1;
  const size_t n_valid_first = sp.parent.size();
  if (!mplx_shim::poly2_space_fetch(p, 0, epoch, res, true, sp, "getAllPrimitives()")) return 1;
  // a second planner plans on the shared device object: the first planner's space is gone
  double start2[9] = {0.5, 4, 0, 0, 0, 0, 0, 0, 0};
  mplx_result res2 = mplx_result();
  if (!ok(p, mplx_poly_plan_batch(p, 1, &world, start2, goal, EPS, TOL_POS, -1.0, 200, 1, &res2))) return 1;
  mplx_shim::Poly2Space again;
  const bool served = mplx_shim::poly2_space_fetch(p, 0, epoch, res, true, again, "getCloseSet()");
  printf("{\"status\": %d, \"n_nodes\": %llu, \"n_expanded\": %llu, \"valid\": %zu, \"valid_first\": %zu, \"all\": %zu, ", res.status, (unsigned long long)res.n_nodes,
         (unsigned long long)res.n_expanded, sp.parent.size(), n_valid_first, sp.parent.size() + sp.blocked_parent.size());
  print_array("close_set", sp.positions(1)); printf(", ");
  print_array("open_set", sp.positions(0)); printf(", ");
  print_array("expanded_nodes", sp.positions(2));
  printf(", \"served_after_other_plan\": %d, \"after_close\": %zu, \"after_open\": %zu, \"after_expanded\": %zu, \"after_valid\": %zu, \"after_all\": %zu}\n", served ? 1 : 0,
         again.positions(1).size(), again.positions(0).size(), again.positions(2).size(), again.parent.size(), again.parent.size() + again.blocked_parent.size());
  return 0;
}

int run_lpa(mplx_poly *p) {
  mplx_plpa *l = nullptr;
  if (!setup(p) || mplx_plpa_create(p, &l) != MPLX_OK) return 1;
  mplx_plpa_set_capacity(l, 1u << 18, 1u << 20, 1u << 20);
  double start[9] = {0.5, 10, 0, 0, 0, 0, 0, 0, 0}, goal[9] = {19, 10, 0, 0, 0, 0, 0, 0, 0};
  std::string out = "{\"ticks\": [";
  int rc = 0;
  for (int tick = 0; tick < 3 && rc == 0; tick++) {
    const double t = DT * tick;
    start[8] = t;
    if (!world_at(p, t)) { rc = 1; break; }
    uint64_t nb = 0, nc = 0;
    if (mplx_plpa_initialized(l) && mplx_plpa_update_nodes(l, 0, &nb, &nc) != MPLX_OK) { printf("error: %s\n", mplx_plpa_last_error(l)); rc = 1; break; }
    mplx_result res = mplx_result();
    if (mplx_plpa_plan(l, 0, start, goal, EPS, TOL_POS, -1.0, MAX_EXPAND, 1, &res) != MPLX_OK) { printf("error: %s\n", mplx_plpa_last_error(l)); rc = 1; break; }
    mplx_shim::Poly2Space sp;
    if (!mplx_shim::poly2_space_fetch_lpa(l, res, sp)) { rc = 1; break; }
    // the counts, from the entries directly
    uint64_t n = 0, ne = 0;
    mplx_plpa_counts(l, &n, &ne);
    std::vector<int32_t> closed((size_t)n + 1), opened((size_t)n + 1), blocked((size_t)ne + 1), ids((size_t)res.n_expanded + 1);
    uint32_t n_rec = 0;
    if (mplx_plpa_result_nodes(l, n, nullptr, nullptr, nullptr, nullptr, closed.data(), opened.data(), nullptr) != MPLX_OK ||
        mplx_plpa_result_entries(l, ne, nullptr, nullptr, nullptr, blocked.data()) != MPLX_OK ||
        mplx_plpa_result_expanded(l, (uint32_t)res.n_expanded, ids.data(), &n_rec) != MPLX_OK) { printf("error: %s\n", mplx_plpa_last_error(l)); rc = 1; break; }
    size_t c_closed = 0, c_open = 0, c_valid = 0;
    for (size_t i = 0; i < (size_t)n; i++) { c_closed += closed[i] != 0; c_open += opened[i] != 0 && closed[i] == 0; }
    for (size_t i = 0; i < (size_t)ne; i++) c_valid += blocked[i] == 0;
    char buf[512];
    snprintf(buf, sizeof(buf), "%s{\"status\": %d, \"getters\": [%zu, %zu, %zu, %zu, %zu], \"counts\": [%zu, %zu, %u, %zu, %llu], \"update\": [%llu, %llu]}", tick ? ", " : "", res.status,
             sp.positions(1).size() / 2, sp.positions(0).size() / 2, sp.positions(2).size() / 2, sp.parent.size(), sp.parent.size() + sp.blocked_parent.size(), c_closed, c_open, n_rec,
             c_valid, (unsigned long long)ne, (unsigned long long)nb, (unsigned long long)nc);
    out += buf;
    if (res.status != MPLX_PLAN_OK || mplx_plpa_traj_len(l) < 2) break;
    // the robot moves on along its trajectory: re-root at its second state (getSubStateSpace(1)), plan from there next tick
    const int len = mplx_plpa_traj_len(l);
    std::vector<int32_t> act((size_t)len), nid((size_t)len + 1);
    std::vector<double> st((size_t)(len + 1) * 9);
    if (mplx_plpa_result_traj(l, act.data(), nid.data(), st.data()) != MPLX_OK || mplx_plpa_sub_state_space(l, 0, 1) != MPLX_OK) { printf("error: %s\n", mplx_plpa_last_error(l)); rc = 1; break; }
    memcpy(start, &st[9], sizeof(double) * 9);
  }
  mplx_plpa_destroy(l);
  if (rc == 0) printf("%s]}\n", out.c_str());
  return rc;
}
}  // namespace

int main(int argc, char **argv) {
  mplx_poly *p = nullptr;
  if (mplx_poly_create(0, &p) != MPLX_OK) {
    printf("%s\n", mplx_poly_last_error(nullptr));
    return 3;
  }
  const int rc = (argc > 1 && std::string(argv[1]) == "lpa") ? run_lpa(p) : run_astar(p);
  mplx_poly_destroy(p);
  return rc;
}
