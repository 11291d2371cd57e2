// mplx_poly_lpa_handle.h -- the mplx_plpa handle and the steps of its calls that the single-planner entries (mplx_poly_lpa.hip) and
// the fleet entries (mplx_poly_lpa_fleet.hip) share: the fresh-or-repair decision, the per-handle kernel arguments, what is done with
// the results of a launch.  Host only; the functions are defined in mplx_poly_lpa.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/mplx.h"
#include "mplx_poly_lpa.h"
#include "mplx_poly_lpa_host.h"
#include "mplx_plpa_space.h"

struct mplx_plpa {
  mplx_poly *poly = nullptr;
  std::string err;
  // capacities and pools (flat, private to the handle: chunk tables are the identity)
  uint64_t cap_nodes = 1 << 18, cap_edges = 1 << 21, cap_log = 1 << 21;
  bool pools_valid = false;
  int pool_control = 0;
  char *node_pool = nullptr, *edge_pool = nullptr, *open_pool = nullptr;
  unsigned long long *table = nullptr;
  uint64_t table_slots = 0;
  uint32_t *bkt_head = nullptr;
  mplx::LpaState *d_st = nullptr;
  mplx::QueryIn *d_in = nullptr;
  mplx::QueryOut *d_out = nullptr;
  int32_t *d_traj_nodes = nullptr, *d_traj_actions = nullptr, *d_rec = nullptr;
  double *d_traj_states = nullptr;
  uint32_t *d_changed = nullptr, *d_counters = nullptr;
  double *d_edge_cost = nullptr;
  uint32_t *d_succ_child = nullptr, *d_succ_entry = nullptr;  // per state x control input (null when that would be too large)
  int succ_n_u = 0;
  uint64_t synced_epoch = ~0ull;  // mplx_poly commit count the entries' blocked bits were last brought in step with
  uint32_t cap_rec = 0;
  // a member of a fleet: d_st / d_in / d_out / d_counters are these slices of the fleet's arrays (not the handle's to free)
  mplx::LpaState *fleet_st = nullptr;
  mplx::QueryIn *fleet_in = nullptr;
  mplx::QueryOut *fleet_out = nullptr;
  uint32_t *fleet_counters = nullptr;
  bool in_fleet = false;  // owned by a fleet: mplx_plpa_destroy ignores it
  // host copies
  mplx::LpaState st{};
  mplx::QueryOut last_out{};
  bool valid = false;
  double goal[9] = {0}, eps = 1.0, tol_pos = 0.5, tol_vel = -1.0;
  int32_t max_expand = -1, heur_ignore_dynamics = 1;
  int32_t root_key[mplx::MAX_KEY + 1] = {0};
  int traj_len = 0;
  std::vector<int32_t> traj_nodes, traj_actions;
  std::vector<double> traj_states;
  std::vector<uint32_t> changed;
  float last_ms = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  mplx_plpa_space *space = nullptr;  // scratch of the state-space exports (mplx_plpa_space.hip)
};

// the query of one plan() and the decision it starts with
struct PlpaQuery {
  mplx::QueryIn in;
  int32_t key[mplx::MAX_KEY + 1];  // of the start state (time-keyed)
  bool fresh;                      // a new state space is started (else the one of the last plan is repaired)
};

// the planner set-up of a plan() call; a space that was built under another eps / tolerance / heuristic mode is given up
void plpa_setup(mplx_plpa *l, double eps, double tol_pos, double tol_vel, int32_t max_expand, int32_t heur_ignore_dynamics);
// pools for this control kind and lattice width (allocated on the first call and after mplx_plpa_set_capacity)
int plpa_ensure(mplx_plpa *l, int control, int n_u);
// MPLX_ERR_ARG when the poly handle is not committed, or its set-up is not one the LPA* runs (control kind, lattice width)
int plpa_poly_view(mplx_poly *poly, std::string *err, mplx_poly_view &v);
// L6: the space of the last plan is repaired when it is valid, the goal is the same and the start is its root
void plpa_query(const mplx_plpa *l, int control, const double *start, const double *goal, bool force_fresh, PlpaQuery &q);
void plpa_params(const mplx_plpa *l, const mplx_poly_view &v, mplx::SearchParams &P);
// PlpaArgs of a plan launch; a fresh space is in step with the world as committed now (synced_epoch)
void plpa_plan_args(mplx_plpa *l, const mplx_poly_view &v, int32_t world, bool fresh, mplx::PlpaArgs &A);
// after a plan launch, l->last_out and l->st hold the results: fills `out`, keeps or drops the space, fetches the trajectory
// (s != nullptr: with asynchronous copies on s, which the caller waits for)
int plpa_plan_finish(mplx_plpa *l, const PlpaQuery &q, const double *goal, mplx_result *out, hipStream_t s);
// PlpaArgs of an updateNodes launch
void plpa_update_args(const mplx_plpa *l, int32_t world, const mplx::SearchParams &P, mplx::PlpaArgs &A);
// after an updateNodes launch, with its counters: the changed entries are fetched (s != nullptr: asynchronously on s; the caller waits
// and calls plpa_changed_sort)
int plpa_update_finish(mplx_plpa *l, const uint32_t ctr[4], uint32_t changed_cap, uint64_t commit_epoch, uint64_t *n_blocked, uint64_t *n_cleared, hipStream_t s);
void plpa_changed_sort(mplx_plpa *l);
int plpa_update_grid(const mplx_plpa *l);  // workgroups of an updateNodes walk over the handle's states
// wait for the stream with the poly handle's launch deadline (opt-in, counted from `t0`): past it the abort word of the planner
// context's guard block is raised, which plpa_plan_kernel polls
int plpa_wait(std::string *err, const mplx_poly_view &v, std::chrono::steady_clock::time_point t0, const char *what);
