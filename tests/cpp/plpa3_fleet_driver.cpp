// plpa3_fleet_driver.cpp -- a fleet of 8 LPA* planners of the 3-D moving-obstacle environment through the plain C-ABI (include/mplx.h,
// mplx_poly3_* and mplx_plpa3_fleet_*): no reference header, no shim class.  The worlds are built in code as
// mpl_ros_amd/poly_map3d.py's replanner_world3 builds them (five 2 m cubes moving at constant velocity in a 20 m x 20 m x 4 m box;
// world 1: from t = 2 on the last cube moves the other way and the second one stops); the members are the four ACC pairs of
// tests/test_poly3_lpa_fleet.py, each in world 0 and in world 1.  Five ticks of the replanner flow: the worlds at t, updateNodes, plan,
// getSubStateSpace(1), on from the second state of the trajectory.  Prints one JSON line per tick; exit 3 and "no HIP device" without
// a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mplx.h"

static const int N = 8, TICKS = 5;
static const double PAIRS[4][6] = {{4, 10, 2, 19, 10, 2}, {5, 2, 2, 12, 18, 2}, {2, 9, 1, 15, 9, 3}, {9, 2, 3, 9, 18, 1}};  // start position, goal position
static const double OBS[5][6] = {{6, 12, 1.5, 0, -0.6, 0}, {10, 6, 2.5, 0, 0.5, 0}, {13, 14, 2, -0.3, -0.7, 0}, {16, 9, 1.25, 0, 0.4, 0.1},
                                 {8, 9.5, 2.75, 0.4, 0.0, -0.1}};  // centre at t = 0, velocity

#define CHECK(call, what)                                                  \
  do {                                                                     \
    int r__ = (call);                                                      \
    if (r__ != MPLX_OK) {                                                  \
      printf("%s failed (%d): %s\n", #call, r__, (what));                  \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int set_worlds(mplx_poly3 *p, double t) {
  // the 2 m cube: rows {px, py, pz, nx, ny, nz}
  const double cube[36] = {-1.0, 0, 0, -1, -0.0, -0.0, 1.0, 0, 0, 1, 0, 0, 0, -1.0, 0, -0.0, -1, -0.0, 0, 1.0, 0, 0, 1, 0, 0, 0, -1.0, -0.0, -0.0, -1, 0, 0, 1.0, 0, 0, 1};
  const double ori[3] = {0.0, 0.0, 0.0}, dim[3] = {20.0, 20.0, 4.0};
  CHECK(mplx_poly3_begin(p, 2), mplx_poly3_last_error(p));
  for (int w = 0; w < 2; w++) {
    CHECK(mplx_poly3_set_world(p, w, ori, dim, t), mplx_poly3_last_error(p));
    for (int k = 0; k < 5; k++) {
      double v[3] = {OBS[k][3], OBS[k][4], OBS[k][5]}, pos[3];
      for (int a = 0; a < 3; a++) pos[a] = OBS[k][a] + v[a] * t;
      if (w == 1 && t >= 2.0) {
        if (k == 4)
          for (int a = 0; a < 3; a++) { pos[a] = OBS[k][a] + v[a] * 2.0 - v[a] * (t - 2.0); v[a] = -v[a]; }
        if (k == 1)
          for (int a = 0; a < 3; a++) { pos[a] = OBS[k][a] + v[a] * 2.0; v[a] = 0 * v[a]; }
      }
      CHECK(mplx_poly3_add_linear(p, w, 6, cube, pos, v, 0.2), mplx_poly3_last_error(p));
    }
  }
  CHECK(mplx_poly3_commit(p), mplx_poly3_last_error(p));
  return 0;
}

int main() {
  mplx_poly3 *p = nullptr;
  if (mplx_poly3_create(0, &p) != MPLX_OK) {
    printf("no HIP device: %s\n", mplx_poly3_last_error(nullptr));
    return 3;
  }
  std::vector<double> U;
  for (double x = -1.0; x <= 1.0; x += 1.0)
    for (double y = -1.0; y <= 1.0; y += 1.0)
      for (double z = -1.0; z <= 1.0; z += 1.0) {
        U.push_back(x); U.push_back(y); U.push_back(z);
      }
  CHECK(mplx_poly3_config(p, MPLX_ACC, 27, U.data(), 1.0, 2.0, 1.0, -1.0, 10.0), mplx_poly3_last_error(p));
  CHECK(mplx_poly3_set_deadline(p, 120.0), mplx_poly3_last_error(p));
  if (set_worlds(p, 0.0)) return 1;

  int32_t world_of[N];
  double starts[N * 13], goals[N * 13];
  memset(starts, 0, sizeof(starts));
  memset(goals, 0, sizeof(goals));
  for (int i = 0; i < N; i++) {
    world_of[i] = i & 1;
    for (int a = 0; a < 3; a++) {
      starts[13 * i + a] = PAIRS[i / 2][a];
      goals[13 * i + a] = PAIRS[i / 2][3 + a];
    }
  }
  mplx_plpa3_fleet *f = nullptr;
  CHECK(mplx_plpa3_fleet_create(p, N, world_of, &f), "fleet");
  if (mplx_plpa3_fleet_size(f) != N) return 1;
  CHECK(mplx_plpa3_fleet_set_capacity(f, 1 << 15, 1 << 18, 1 << 18), mplx_plpa3_fleet_last_error(f));
  double t = 0.0;
  for (int tick = 0; tick < TICKS; tick++) {
    if (set_worlds(p, t)) return 1;
    uint64_t nb[N], nc[N];
    CHECK(mplx_plpa3_fleet_update_nodes(f, nb, nc), mplx_plpa3_fleet_last_error(f));
    mplx_result res[N];
    CHECK(mplx_plpa3_fleet_plan(f, starts, goals, nullptr, 1.0, 0.5, -1.0, 5000, 1, res), mplx_plpa3_fleet_last_error(f));
    uint32_t st[4];
    CHECK(mplx_plpa3_fleet_stats(f, st), "stats");
    printf("{\"tick\": %d, \"stats\": [%u, %u, %u, %u], \"members\": [", tick, st[0], st[1], st[2], st[3]);
    int32_t steps[N];
    for (int i = 0; i < N; i++) {
      mplx_plpa3 *m = mplx_plpa3_fleet_member(f, i);
      uint64_t cost_bits = 0;
      memcpy(&cost_bits, &res[i].cost, 8);
      const int len = mplx_plpa3_traj_len(m);
      printf("%s{\"status\": %d, \"cost_bits\": %llu, \"n_expanded\": %llu, \"expand_hash\": %llu, \"traj_len\": %d, \"blocked\": %llu, \"cleared\": %llu}", i ? ", " : "",
             res[i].status, (unsigned long long)cost_bits, (unsigned long long)res[i].n_expanded, (unsigned long long)res[i].expand_hash, len,
             (unsigned long long)nb[i], (unsigned long long)nc[i]);
      steps[i] = -1;
      if (res[i].status == MPLX_PLAN_OK && len > 2) {  // on from the second state of the trajectory
        std::vector<double> states((size_t)(len + 1) * 13);
        CHECK(mplx_plpa3_result_traj(m, nullptr, nullptr, states.data()), mplx_plpa3_last_error(m));
        memcpy(&starts[13 * i], &states[13], sizeof(double) * 13);
        starts[13 * i + 12] = t + 1.0;
        steps[i] = 1;
      }
    }
    printf("]}\n");
    CHECK(mplx_plpa3_fleet_sub_state_space(f, steps), mplx_plpa3_fleet_last_error(f));
    t += 1.0;
  }
  mplx_plpa3_fleet_destroy(f);
  mplx_poly3_destroy(p);
  return 0;
}
