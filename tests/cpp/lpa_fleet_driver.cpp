// lpa_fleet_driver.cpp -- a fleet of 4 LPA* planners through the plain C-ABI (include/mplx.h, mplx_lpa_fleet_*): no reference
// header, no shim class.  The map is built in code (tests/test_lpa_fleet.py builds the same one): 160 x 120 x 1 cells of 0.1 m,
// two walls with gaps; four robots plan across it, a bar of cells is blocked between the walls (updateBlockedNodes, plan), then
// freed again (updateClearedNodes, plan).  Prints one JSON line; exit 3 and "no HIP device" without a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mplx.h"

static const int DX = 160, DY = 120, DZ = 1, N = 4;
static const int PAIRS[N][4] = {{10, 10, 150, 100}, {150, 20, 10, 110}, {20, 100, 140, 10}, {80, 10, 80, 110}};  // start cell, goal cell

static mplx_waypoint wp(int ix, int iy) {
  mplx_waypoint w;
  memset(&w, 0, sizeof(w));
  w.pos[0] = (ix + 0.5) * 0.1;
  w.pos[1] = (iy + 0.5) * 0.1;
  w.pos[2] = 0.025;
  w.control = MPLX_ACC;
  return w;
}

#define CHECK(call, what)                                                                      \
  do {                                                                                         \
    int r__ = (call);                                                                          \
    if (r__ != MPLX_OK) {                                                                      \
      printf("%s failed (%d): %s | %s\n", #call, r__, mplx_last_error(ctx), (what));           \
      return 1;                                                                                \
    }                                                                                          \
  } while (0)

int main() {
  mplx_ctx *ctx = nullptr;
  if (mplx_ctx_create(0, &ctx) != MPLX_OK) {
    printf("no HIP device: %s\n", mplx_last_error(nullptr));
    return 3;
  }
  std::vector<int8_t> grid((size_t)DX * DY * DZ, 0);
  for (int y = 0; y < 70; y++)
    for (int x = 50; x < 55; x++) grid[(size_t)x + (size_t)DX * y] = 100;
  for (int y = 50; y < DY; y++)
    for (int x = 100; x < 105; x++) grid[(size_t)x + (size_t)DX * y] = 100;
  const int32_t dim[3] = {DX, DY, DZ};
  const double origin[3] = {0.0, 0.0, 0.0};
  CHECK(mplx_map_set(ctx, grid.data(), dim, origin, 0.1), "map");
  // the 2-D lattice of 9 inputs: x outermost, u = 1, accumulated like the reference driver
  std::vector<double> U;
  for (double x = -1.0; x <= 1.0; x += 1.0)
    for (double y = -1.0; y <= 1.0; y += 1.0) {
      U.push_back(x); U.push_back(y); U.push_back(0.0);
    }
  mplx_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.control = MPLX_ACC;
  cfg.n_u = (int32_t)(U.size() / 3);
  cfg.U = U.data();
  cfg.dt = 1.0; cfg.v_max = 2.0; cfg.a_max = 1.0; cfg.j_max = -1.0;
  cfg.w = 10.0; cfg.eps = 1.0;
  cfg.tol_pos = 0.5; cfg.tol_vel = 1.0; cfg.tol_acc = 1.0;
  cfg.t_max = INFINITY;
  cfg.max_expand = -1;
  cfg.yaw_max = -1.0; cfg.tol_yaw = -1.0;
  CHECK(mplx_planner_config(ctx, &cfg), "config");
  CHECK(mplx_set_capacity(ctx, 1, 1 << 17, 1 << 19, 1 << 19), "capacity");
  CHECK(mplx_set_deadline(ctx, 120.0), "deadline");

  mplx_lpa_fleet *f = nullptr;
  CHECK(mplx_lpa_fleet_create(ctx, N, &f), "fleet");
  if (mplx_lpa_fleet_size(f) != N) return 1;
  CHECK(mplx_lpa_fleet_set_capacity(f, 1 << 17, 1 << 19, 1 << 19), mplx_lpa_fleet_last_error(f));
  mplx_waypoint starts[N], goals[N];
  for (int i = 0; i < N; i++) {
    starts[i] = wp(PAIRS[i][0], PAIRS[i][1]);
    goals[i] = wp(PAIRS[i][2], PAIRS[i][3]);
  }
  std::vector<int32_t> cells;  // the bar between the walls
  for (int y = 55; y < 60; y++)
    for (int x = 70; x < 90; x++) {
      cells.push_back(x); cells.push_back(y); cells.push_back(0);
    }
  printf("{\"steps\": [");
  for (int step = 0; step < 3; step++) {
    uint64_t changed[N] = {0, 0, 0, 0};
    if (step > 0) {
      const int8_t v = step == 1 ? 100 : 0;
      for (size_t k = 0; k < cells.size(); k += 3) grid[(size_t)cells[k] + (size_t)DX * cells[k + 1]] = v;
      CHECK(mplx_map_set(ctx, grid.data(), dim, origin, 0.1), "map edit");
      if (step == 1) CHECK(mplx_lpa_fleet_update_blocked(f, (int)(cells.size() / 3), cells.data(), changed), mplx_lpa_fleet_last_error(f));
      else CHECK(mplx_lpa_fleet_update_cleared(f, (int)(cells.size() / 3), cells.data(), changed), mplx_lpa_fleet_last_error(f));
    }
    mplx_result res[N];
    CHECK(mplx_lpa_fleet_plan(f, starts, goals, nullptr, res), mplx_lpa_fleet_last_error(f));
    uint32_t st[4];
    CHECK(mplx_lpa_fleet_stats(f, st), "stats");
    printf("%s{\"stats\": [%u, %u, %u, %u], \"members\": [", step ? ", " : "", st[0], st[1], st[2], st[3]);
    for (int i = 0; i < N; i++) {
      mplx_lpa *m = mplx_lpa_fleet_member(f, i);
      uint64_t nn = 0, ne = 0, nb = 0, cost_bits = 0;
      CHECK(mplx_lpa_counts(m, &nn, &ne, &nb), mplx_lpa_last_error(m));
      memcpy(&cost_bits, &res[i].cost, 8);
      printf("%s{\"status\": %d, \"cost_bits\": %llu, \"n_expanded\": %llu, \"expand_hash\": %llu, \"n_nodes\": %llu, \"n_edges\": %llu, \"traj_len\": %d, "
             "\"changed\": %llu, \"initialized\": %d, \"space_nodes\": %llu, \"space_edges\": %llu, \"blocked_log\": %llu}",
             i ? ", " : "", res[i].status, (unsigned long long)cost_bits, (unsigned long long)res[i].n_expanded, (unsigned long long)res[i].expand_hash,
             (unsigned long long)res[i].n_nodes, (unsigned long long)res[i].n_edges, mplx_lpa_traj_len(m), (unsigned long long)changed[i],
             mplx_lpa_initialized(m), (unsigned long long)nn, (unsigned long long)ne, (unsigned long long)nb);
    }
    printf("]}");
  }
  printf("]}\n");
  mplx_lpa_fleet_destroy(f);
  mplx_ctx_destroy(ctx);
  return 0;
}
