// poly_space_checker.cpp -- the CPU checker of the moving-obstacle environment (poly_checker.cpp, included unchanged) with exports for
// what its search keeps per node and poly_checker.cpp does not hand out: the predecessor lists (pred / pact, in push_back order), and,
// in bulk, the states, values and flags of all nodes and the blocked primitives of the closed ones -- the actions for which
// get_succ(node state) returns an infinite cost, closed nodes in id order.  TEST INFRASTRUCTURE ONLY (tests/poly_space_checker.py).
#include "poly_checker.cpp"

namespace {
template <class F2, class F3>
auto with_checker(void *h, F2 f2, F3 f3) -> decltype(f2(*(Checker<2> *)nullptr)) {
  Base *b = (Base *)h;
  if (auto *c = dynamic_cast<Checker<2> *>(b)) return f2(*c);
  return f3(*dynamic_cast<Checker<3> *>(b));
}
template <class C>
int pred_len(const C &c, int id) { return (int)c.nodes[(size_t)id].pred.size(); }
template <class C>
void pred_get(const C &c, int id, int *parent, int *action) {
  const auto &n = c.nodes[(size_t)id];
  for (size_t e = 0; e < n.pred.size(); e++) { parent[e] = n.pred[e]; action[e] = n.pact[e]; }
}
template <class C>
long long pred_all(const C &c, long long cap, int *child, int *parent, int *action) {
  long long w = 0;
  for (size_t i = 0; i < c.nodes.size(); i++)
    for (size_t e = 0; e < c.nodes[i].pred.size(); e++) {
      if (w < cap) { child[w] = (int)i; parent[w] = c.nodes[i].pred[e]; action[w] = c.nodes[i].pact[e]; }
      w++;
    }
  return w;
}
template <class C, int Dim>
void nodes_all(const C &c, double *states, double *g, double *h, int *closed, int *opened) {
  for (size_t i = 0; i < c.nodes.size(); i++) {
    C::to(c.nodes[i].coord, states + (4 * Dim + 1) * i);
    g[i] = c.nodes[i].g; h[i] = c.nodes[i].h; closed[i] = c.nodes[i].closed; opened[i] = c.nodes[i].opened;
  }
}
template <class C, int Dim>
long long blocked_all(C &c, long long cap, int *parent, int *action) {
  long long w = 0;
  vec_E<Waypoint<Dim>> succ;
  std::vector<double> cost;
  std::vector<int> act;
  for (size_t i = 0; i < c.nodes.size(); i++) {
    if (!c.nodes[i].closed) continue;
    c.E.get_succ(c.nodes[i].coord, succ, cost, act);
    for (size_t k = 0; k < succ.size(); k++) {
      if (!std::isinf(cost[k])) continue;
      if (w < cap) { parent[w] = (int)i; action[w] = act[k]; }
      w++;
    }
  }
  return w;
}
}  // namespace

extern "C" {
// predecessor list of node id of the last plan: its length; (parent, action) per record, oldest first
int psc_pred_len(void *h, int id) {
  return with_checker(h, [&](Checker<2> &c) { return pred_len(c, id); }, [&](Checker<3> &c) { return pred_len(c, id); });
}
int psc_pred_get(void *h, int id, int *parent, int *action) {
  return with_checker(h, [&](Checker<2> &c) { pred_get(c, id, parent, action); return 0; }, [&](Checker<3> &c) { pred_get(c, id, parent, action); return 0; });
}
// all lists, children in id order: returns the full count, writes at most cap records
long long psc_pred_all(void *h, long long cap, int *child, int *parent, int *action) {
  return with_checker(h, [&](Checker<2> &c) { return pred_all(c, cap, child, parent, action); }, [&](Checker<3> &c) { return pred_all(c, cap, child, parent, action); });
}
// all nodes: states n x (4 Dim + 1), g, h, closed, opened
int psc_nodes_all(void *h, double *states, double *g, double *hh, int *closed, int *opened) {
  return with_checker(h, [&](Checker<2> &c) { nodes_all<Checker<2>, 2>(c, states, g, hh, closed, opened); return 0; },
                      [&](Checker<3> &c) { nodes_all<Checker<3>, 3>(c, states, g, hh, closed, opened); return 0; });
}
// blocked primitives of the closed nodes, ids ascending, in the order get_succ emits them: full count, at most cap written
long long psc_blocked_all(void *h, long long cap, int *parent, int *action) {
  return with_checker(h, [&](Checker<2> &c) { return blocked_all<Checker<2>, 2>(c, cap, parent, action); },
                      [&](Checker<3> &c) { return blocked_all<Checker<3>, 3>(c, cap, parent, action); });
}
}
