/**
 * @file poly2_space.h  (mplx shim: the state space of PolyMapPlanner<2> from the device)
 *
 * What MPL::PolyMapPlanner<2>'s getCloseSet / getOpenSet / getExpandedNodes / getValidPrimitives / getAllPrimitives
 * (poly_map_planner.h of this shim) answer with, fetched into host vectors with no reference header in sight:
 *   - A* mode: query 0 of the planner's last mplx_poly_plan_batch on the SHARED device object, through
 *     mplx_poly_result_nodes / _edges / _blocked / _expanded.  The object serves every planner of the process, so the fetch
 *     first compares mplx_poly_plan_epoch with the epoch the planner noted after its own plan(): when another planner has
 *     planned there since, the space is gone -- a red refusal, nothing fetched (the rule of MapPlanner::own_results()).
 *   - setLPAstar(true) mode: the planner's own mplx_plpa handle, through mplx_plpa_result_nodes / _expanded / _entries.
 * One copy per plan is kept by the caller (Poly2Space): the five getters of one plan share one fetch; the blocked
 * primitives of an A* plan -- re-derived on the device on request -- are fetched when getAllPrimitives first asks.
 * A program that does not have the reference's headers -- a test driver -- reads the space through this header exactly as
 * the shim's planner does.
 */
#ifndef MPLX_SHIM_POLY2_SPACE_H
#define MPLX_SHIM_POLY2_SPACE_H

#include <mplx.h>

#include <cstdint>
#include <cstdio>
#include <vector>

namespace mplx_shim {

/// the state space of one 2-D plan on the host: states n x 9 (pos2 vel2 acc2 jrk2 t) and flags in id order, the expansion
/// order (node ids), the predecessor records with finite cost (child, parent, action) and the blocked ones (parent, action)
struct Poly2Space {
  bool fetched = false;          // nodes, expansion order and valid records are here
  bool blocked_fetched = false;  // the blocked records too
  std::vector<double> states;
  std::vector<int32_t> closed, opened, expanded;
  std::vector<int32_t> child, parent, action;
  std::vector<int32_t> blocked_parent, blocked_action;
  size_t n_nodes() const { return closed.size(); }
  /// positions (x, y pairs) of: which = 1 the closed states, 0 the states in OPEN (opened and not closed), both in id order
  /// (upstream walks a hash map: its order is unspecified); 2 the expanded states in expansion order
  std::vector<double> positions(int which) const {
    std::vector<double> xy;
    if (which == 2) {
      for (int32_t id : expanded)
        if (id >= 0 && (size_t)id < n_nodes()) { xy.push_back(states[9 * (size_t)id]); xy.push_back(states[9 * (size_t)id + 1]); }
      return xy;
    }
    for (size_t i = 0; i < n_nodes(); i++)
      if (which == 1 ? closed[i] != 0 : (opened[i] != 0 && closed[i] == 0)) { xy.push_back(states[9 * i]); xy.push_back(states[9 * i + 1]); }
    return xy;
  }
};

inline void poly2_refuse(const char *what, const char *why) { printf("\x1b[31m[PolyMapPlanner] %s refused: %s\n\x1b[0m", what, why); }
inline bool poly2_check(mplx_poly *p, int rc) {
  if (rc == MPLX_OK) return true;
  printf("\x1b[31m[PolyMapPlanner] %s\n\x1b[0m", mplx_poly_last_error(p));
  return false;
}
/// the planner's plan is still the last one of the shared device object
inline bool poly2_own_results(mplx_poly *p, uint64_t epoch, const char *what) {
  if (p && epoch != 0 && mplx_poly_plan_epoch(p) == epoch) return true;
  poly2_refuse(what, epoch == 0 ? "this planner has not planned on the device" :
                                  "another planner has planned on the shared device object since this planner's plan(): its state space is gone");
  return false;
}

/// A* mode: query q of the plan the caller noted `epoch` after (mplx_poly_plan_epoch).  with_blocked: the blocked records too.
/// false: refused or a device call failed (the message is printed), `out` is left empty.
inline bool poly2_space_fetch(mplx_poly *p, int32_t q, uint64_t epoch, const mplx_result &res, bool with_blocked, Poly2Space &out, const char *what) {
  if (!poly2_own_results(p, epoch, what)) { out = Poly2Space(); return false; }
  if (!out.fetched) {
    out = Poly2Space();
    const uint64_t n = res.n_nodes;
    if (n > 0) {
      out.states.resize((size_t)n * 9);
      out.closed.resize((size_t)n);
      out.opened.resize((size_t)n);
      if (!poly2_check(p, mplx_poly_result_nodes(p, q, n, out.states.data(), nullptr, nullptr, out.closed.data(), out.opened.data()))) { out = Poly2Space(); return false; }
      uint64_t ne = 0;
      if (!poly2_check(p, mplx_poly_result_edges(p, q, 0, nullptr, nullptr, nullptr, &ne))) { out = Poly2Space(); return false; }
      out.child.resize((size_t)ne); out.parent.resize((size_t)ne); out.action.resize((size_t)ne);
      if (ne && !poly2_check(p, mplx_poly_result_edges(p, q, ne, out.child.data(), out.parent.data(), out.action.data(), &ne))) { out = Poly2Space(); return false; }
    }
    if (res.n_expanded > 0) {
      uint32_t got = 0;
      out.expanded.resize((size_t)res.n_expanded);
      if (!poly2_check(p, mplx_poly_result_expanded(p, q, (uint32_t)out.expanded.size(), out.expanded.data(), &got))) { out = Poly2Space(); return false; }
      out.expanded.resize(got);
    }
    out.fetched = true;
  }
  if (with_blocked && !out.blocked_fetched) {
    uint64_t nb = 0;
    if (!poly2_check(p, mplx_poly_result_blocked(p, q, 0, nullptr, nullptr, &nb))) return false;
    out.blocked_parent.resize((size_t)nb); out.blocked_action.resize((size_t)nb);
    if (nb && !poly2_check(p, mplx_poly_result_blocked(p, q, nb, out.blocked_parent.data(), out.blocked_action.data(), &nb))) {
      out.blocked_parent.clear(); out.blocked_action.clear();
      return false;
    }
    out.blocked_fetched = true;
  }
  return true;
}

/// setLPAstar(true) mode: the space of the planner's own LPA* handle as it is now; entries with blocked == 0 are the valid
/// records, the others the blocked ones.  (Through the host-decoded dumps on purpose: at the few hundred states of a replanner
/// tick their two blocking copies are quicker than the passes of mplx_plpa_export_space / _records, which win from some
/// thousand states on -- measured, DESIGN 3.6.  The changed primitives of updateNodes() do come from the export.)
inline bool poly2_space_fetch_lpa(mplx_plpa *l, const mplx_result &res, Poly2Space &out) {
  if (out.fetched) return true;
  out = Poly2Space();
  if (!l) return false;
  auto ok = [&](int rc) {
    if (rc == MPLX_OK) return true;
    printf("\x1b[31m[PolyMapPlanner] %s\n\x1b[0m", mplx_plpa_last_error(l));
    out = Poly2Space();
    return false;
  };
  uint64_t n = 0, ne = 0;
  if (!ok(mplx_plpa_counts(l, &n, &ne))) return false;
  if (n > 0) {
    out.states.resize((size_t)n * 9);
    out.closed.resize((size_t)n);
    out.opened.resize((size_t)n);
    if (!ok(mplx_plpa_result_nodes(l, n, out.states.data(), nullptr, nullptr, nullptr, out.closed.data(), out.opened.data(), nullptr))) return false;
  }
  if (ne > 0) {
    std::vector<int32_t> c((size_t)ne), pa((size_t)ne), a((size_t)ne), b((size_t)ne);
    if (!ok(mplx_plpa_result_entries(l, ne, c.data(), pa.data(), a.data(), b.data()))) return false;
    for (size_t i = 0; i < (size_t)ne; i++) {
      if (b[i]) { out.blocked_parent.push_back(pa[i]); out.blocked_action.push_back(a[i]); }
      else { out.child.push_back(c[i]); out.parent.push_back(pa[i]); out.action.push_back(a[i]); }
    }
  }
  if (res.n_expanded > 0) {
    uint32_t got = 0;
    out.expanded.resize((size_t)res.n_expanded);
    if (!ok(mplx_plpa_result_expanded(l, (uint32_t)out.expanded.size(), out.expanded.data(), &got))) return false;
    out.expanded.resize(got);
  }
  out.fetched = out.blocked_fetched = true;
  return true;
}

}  // namespace mplx_shim
#endif
