// plpa_fleet_driver.cpp -- a fleet of 16 moving-obstacle LPA* planners through the plain C-ABI (include/mplx.h, mplx_poly_* and
// mplx_plpa_fleet_*): no reference header, no shim class.  The worlds are built in code as mpl_ros_amd/poly_map.py's replanner_world
// builds them (five 2 m boxes moving at constant velocity on a 20 m map; world 1: from t = 2 on the last box moves the other way and
// the second one stops); the members are the eight pairs of tests/golden/plpa_fleet_pairs.json, each in world 0 and in world 1.  Eight
// ticks of the replanner flow: the worlds at t, updateNodes, plan, getSubStateSpace(1), on from the second state of the trajectory.
// Prints one JSON line per tick; exit 3 and "no HIP device" without a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mplx.h"

static const int N = 16, TICKS = 8;
static const double PAIRS[8][4] = {{0.5, 2, 19, 8}, {19.5, 2, 1, 12}, {0.5, 4, 19, 10}, {19.5, 8, 1, 2}, {0.5, 10, 19, 16}, {19.5, 10, 1, 4}, {0.5, 14, 19, 4}, {19.5, 14, 1, 8}};
static const double OBS[5][4] = {{6, 12, 0, -0.6}, {10, 6, 0, 0.5}, {13, 14, -0.3, -0.7}, {16, 9, 0, 0.4}, {8, 9.5, 0.4, 0.0}};  // position at t = 0, velocity

#define CHECK(call, what)                                                  \
  do {                                                                     \
    int r__ = (call);                                                      \
    if (r__ != MPLX_OK) {                                                  \
      printf("%s failed (%d): %s\n", #call, r__, (what));                  \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int set_worlds(mplx_poly *p, double t) {
  const double rec[16] = {-1.0, 0, -1, -0.0, 1.0, 0, 1, 0, 0, -1.0, -0.0, -1, 0, 1.0, 0, 1};  // the 2 m box: rows {px, py, nx, ny}
  const double ori[2] = {0.0, 0.0}, dim[2] = {20.0, 20.0};
  CHECK(mplx_poly_begin(p, 2), mplx_poly_last_error(p));
  for (int w = 0; w < 2; w++) {
    CHECK(mplx_poly_set_world(p, w, ori, dim, t), mplx_poly_last_error(p));
    for (int k = 0; k < 5; k++) {
      double v[2] = {OBS[k][2], OBS[k][3]}, pos[2];
      for (int a = 0; a < 2; a++) pos[a] = OBS[k][a] + v[a] * t;
      if (w == 1 && t >= 2.0) {
        if (k == 4)
          for (int a = 0; a < 2; a++) { pos[a] = OBS[k][a] + v[a] * 2.0 - v[a] * (t - 2.0); v[a] = -v[a]; }
        if (k == 1)
          for (int a = 0; a < 2; a++) { pos[a] = OBS[k][a] + v[a] * 2.0; v[a] = 0 * v[a]; }
      }
      CHECK(mplx_poly_add_linear(p, w, 4, rec, pos, v, 0.2), mplx_poly_last_error(p));
    }
  }
  CHECK(mplx_poly_commit(p), mplx_poly_last_error(p));
  return 0;
}

int main() {
  mplx_poly *p = nullptr;
  if (mplx_poly_create(0, &p) != MPLX_OK) {
    printf("no HIP device: %s\n", mplx_poly_last_error(nullptr));
    return 3;
  }
  std::vector<double> U;
  for (double x = -1.0; x <= 1.0; x += 1.0)
    for (double y = -1.0; y <= 1.0; y += 1.0) {
      U.push_back(x); U.push_back(y);
    }
  CHECK(mplx_poly_config(p, MPLX_ACC, 9, U.data(), 1.0, 2.0, 1.0, -1.0, 10.0), mplx_poly_last_error(p));
  CHECK(mplx_poly_set_deadline(p, 120.0), mplx_poly_last_error(p));
  if (set_worlds(p, 0.0)) return 1;

  int32_t world_of[N];
  double starts[N * 9], goals[N * 9];
  memset(starts, 0, sizeof(starts));
  memset(goals, 0, sizeof(goals));
  for (int i = 0; i < N; i++) {
    world_of[i] = i & 1;
    starts[9 * i] = PAIRS[i / 2][0]; starts[9 * i + 1] = PAIRS[i / 2][1];
    goals[9 * i] = PAIRS[i / 2][2]; goals[9 * i + 1] = PAIRS[i / 2][3];
  }
  mplx_plpa_fleet *f = nullptr;
  CHECK(mplx_plpa_fleet_create(p, N, world_of, &f), "fleet");
  if (mplx_plpa_fleet_size(f) != N) return 1;
  CHECK(mplx_plpa_fleet_set_capacity(f, 1 << 15, 1 << 18, 1 << 18), mplx_plpa_fleet_last_error(f));
  double t = 0.0;
  for (int tick = 0; tick < TICKS; tick++) {
    if (set_worlds(p, t)) return 1;
    uint64_t nb[N], nc[N];
    CHECK(mplx_plpa_fleet_update_nodes(f, nb, nc), mplx_plpa_fleet_last_error(f));
    mplx_result res[N];
    CHECK(mplx_plpa_fleet_plan(f, starts, goals, nullptr, 1.0, 0.5, -1.0, 5000, 1, res), mplx_plpa_fleet_last_error(f));
    uint32_t st[4];
    CHECK(mplx_plpa_fleet_stats(f, st), "stats");
    printf("{\"tick\": %d, \"stats\": [%u, %u, %u, %u], \"members\": [", tick, st[0], st[1], st[2], st[3]);
    int32_t steps[N];
    for (int i = 0; i < N; i++) {
      mplx_plpa *m = mplx_plpa_fleet_member(f, i);
      uint64_t cost_bits = 0;
      memcpy(&cost_bits, &res[i].cost, 8);
      const int len = mplx_plpa_traj_len(m);
      printf("%s{\"status\": %d, \"cost_bits\": %llu, \"n_expanded\": %llu, \"expand_hash\": %llu, \"traj_len\": %d, \"blocked\": %llu, \"cleared\": %llu}", i ? ", " : "",
             res[i].status, (unsigned long long)cost_bits, (unsigned long long)res[i].n_expanded, (unsigned long long)res[i].expand_hash, len,
             (unsigned long long)nb[i], (unsigned long long)nc[i]);
      steps[i] = -1;
      if (res[i].status == MPLX_PLAN_OK && len > 2) {  // on from the second state of the trajectory
        std::vector<double> states((size_t)(len + 1) * 9);
        CHECK(mplx_plpa_result_traj(m, nullptr, nullptr, states.data()), mplx_plpa_last_error(m));
        memcpy(&starts[9 * i], &states[9], sizeof(double) * 9);
        starts[9 * i + 8] = t + 1.0;
        steps[i] = 1;
      }
    }
    printf("]}\n");
    CHECK(mplx_plpa_fleet_sub_state_space(f, steps), mplx_plpa_fleet_last_error(f));
    t += 1.0;
  }
  mplx_plpa_fleet_destroy(f);
  mplx_poly_destroy(p);
  return 0;
}
