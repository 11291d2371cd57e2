// mplx_search_steps.h -- the per-query steps that every one-query-per-workgroup A* kernel runs around its environment:
// reset, admission of the start, the start node, the duplicate probe of an expansion, the termination tests, and
// recoverTraj with the result record.  astar_kernel, astar_spec_kernel (mplx_spec.h), astar_poly_kernel
// (mplx_poly_search.h), astar_cloud_kernel (mplx_cloud.h) and astar_poly3_kernel (mplx_poly3.h) call them; what a kernel
// supplies is its environment: the start test, the goal predicate, get_succ with the lane's edge cost, and the edge cost
// of a stored predecessor record.  Included from mplx_kernels.h (behind QView, open_push and pop_min); the LPA* kernels
// walk their predecessor records differently (blocked edges, stored costs, a root) and do not use this file.
#pragma once

namespace mplx {

// State record fields are written / read with plain accesses unless a kernel says otherwise (the speculative kernel's
// HELP builds: agent scope, for the helper workgroups)
struct PlainStore {
  __device__ __forceinline__ void operator()(double *p, double v) const { *p = v; }
};
struct PlainLoad {
  __device__ __forceinline__ double operator()(const double *p) const { return *p; }
};

// PlannerBase::plan's start test of the voxel environment: the start's cell lies inside the map and is free
__device__ __forceinline__ bool voxel_start_free(const SearchParams &P, const QueryIn &in) {
  int32_t c[3];
  for (int ax = 0; ax < 3; ax++) {
    c[ax] = float_to_cell(in.start.p[ax], P.map.origin[ax], P.map.res);
    if (c[ax] < 0 || c[ax] >= P.map.dim[ax]) return false;
  }
  return P.map.data[(size_t)c[0] + (size_t)P.map.dim[0] * c[1] + (size_t)P.map.dim[0] * P.map.dim[1] * c[2]] == 0;
}

// ---- 1. reset (block-wide; no barrier): the workgroup's OPEN structure, the query's counters and S.hp, the LDS copy of
// the goal and the heuristic parameters.  reserve: near-set room one iteration of the kernel may need.  goal_yaw is read
// by yaw-carrying searches only (the host leaves it 0 otherwise).
template <int BLOCK, int CONTROL, class SM>
__device__ __forceinline__ void query_reset(const QView<BLOCK, CONTROL, SM> &Q, const QueryIn &in, uint32_t reserve, int tid) {
  const SearchParams &P = Q.P;
  SM &S = Q.S;
  for (int i = tid; i < 2 * NB; i += BLOCK) S.cnt[0][i] = 0;
  if (tid == 0) {
    S.n_near = 0; S.n_nodes = 0; S.n_edges = 0; S.n_log = 0;
    S.reserve = reserve;
    S.node_chunks = S.edge_chunks = S.open_chunks = 0;
    S.cur1 = 0; S.cur0 = 0; S.lo1 = 0.0; S.ts_f = INFINITY; S.ts_g = INFINITY; S.ts_id = 0xFFFFFFFFu;
    S.status = -1;
    for (int i = 0; i < 10; i++) S.cyc[i] = 0;
    S.c_expanded = S.c_closed = S.c_prims = S.c_succ = S.c_succ_finite = S.c_reads = 0;
    S.c_push = S.c_reopen = S.c_refill = S.c_evict = 0;
    S.c_hash = 0;
    S.hp.w = P.w; S.hp.v_max = P.v_max; S.hp.heur_ignore_dynamics = P.heur_ignore_dynamics;
    S.hp.goal_control = in.goal_control;
    S.hp.goal = in.goal;
    S.hp.goal_nkey = state_key(in.goal_control, in.goal, S.hp.goal_key);
    S.hp.goal_yaw = in.goal_yaw;
    S.hp.goal_yaw_key = (int32_t)round(in.goal_yaw / KEY_RES_YAW);
  }
}

// ---- 2. admission (thread 0, after query_reset).  PlannerBase::plan: the start must be free (status 2); Astar: a start
// at the goal or past t_max is a plan of cost 0 (status 0, S.tmp_d0).  An admitted query gets its first node and OPEN
// chunk (status 4: the pools are exhausted) and keeps status -1.
template <int BLOCK, int CONTROL, class SM>
__device__ __forceinline__ void query_admit(const QView<BLOCK, CONTROL, SM> &Q, const QueryIn &in, bool start_free, bool at_goal) {
  SM &S = Q.S;
  double cost0 = INFINITY;
  if (!start_free)
    S.status = 2;
  else if (in.start_t >= Q.P.t_max || at_goal) {
    S.status = 0;
    cost0 = 0.0;
  }
  S.tmp_d0 = cost0;
  if (S.status < 0 && !(Q.ensure_nodes(1) && Q.ensure_open(1))) S.status = 4;
}

// ---- 3. start node, id 0 (block-wide, behind the barrier that follows the admission): key, record, heuristic, its slot
// in the shared hash table, f_base, the first OPEN entry.  NK key integers, of which extra_key is the last when NK exceeds
// the state's own (yaw key; round(t / 0.1) of the time-keyed searches); EX extra state doubles (the yaw) ahead of the time.
// heur(key): the start's heuristic.  False when the table had no slot (status 5): the caller must not search.
template <int NK, int EX, int BLOCK, int CONTROL, class SM, class Heur, class Store = PlainStore>
__device__ __forceinline__ bool query_start(const QView<BLOCK, CONTROL, SM> &Q, const QueryIn &in, int q, int tid, int32_t extra_key, double extra_state,
                                            Heur heur, Store store = Store()) {
  using V = QView<BLOCK, CONTROL, SM>;
  const SearchParams &P = Q.P;
  SM &S = Q.S;
  constexpr int ns = key_len_c(CONTROL);
  static_assert(NK == ns || NK == ns + 1, "at most one key integer beyond the state's own");
  if (tid == 0) {
    int32_t key[MAX_KEY + 1];
    state_key_c<CONTROL>(in.start, key);
    if constexpr (NK > ns) key[ns] = extra_key;
    char *rec = Q.node(0);
    for (int i = 0; i < NK; i++) V::key(rec)[i] = key[i];
    const double *src = (const double *)&in.start;
    for (int i = 0; i < ns; i++) store(&V::state(rec)[i], src[i]);
    if constexpr (EX != 0) V::state(rec)[ns] = extra_state;
    V::state(rec)[ns + EX] = in.start_t;
    const double h = P.eps != 0.0 ? heur(key) : 0.0;
    V::h(rec) = h;
    V::g(rec) = 0.0;
    V::flags(rec) = FLAG_OPENED;
    V::pred(rec) = NIL;
    const unsigned long long h64 = key_hash64(key, NK);
    const unsigned long long tagq = tbl_tagq(h64, (uint32_t)q, P.tbl_epoch);
    size_t pos = (size_t)(h64 ^ ((unsigned long long)(uint32_t)q * 0x9E3779B97F4A7C15ull)) & (size_t)P.table_mask;
    for (unsigned long long steps = 0;; steps++) {  // shared table: the home slot may belong to another query
      const unsigned long long seen = ld_u64(&P.table[pos]);  // (a slot of another epoch is empty: claimed against the value seen)
      if (tbl_empty(seen, P.tbl_epoch) && atomicCAS(&P.table[pos], seen, tagq | 0ull) == seen) break;
      if (steps > P.table_mask) { S.status = 5; break; }  // (the table is full: never with the host's sizing)
      pos = (pos + 1) & (size_t)P.table_mask;
    }
    S.n_nodes = 1;
    S.f_base = 0.0 + P.eps * h;
    S.lo1 = S.f_base;
    S.n_log = 1;
    S.c_push = 1;
  }
  __syncthreads();
  if (tid == 0 && S.status < 0) open_push(Q, 0u, S.f_base, 0.0, 0u);
  __syncthreads();
  return S.status < 0;
}

// ---- 4. duplicate probe (block-wide, two barriers): do two control inputs of this expansion reach one key?  An LDS set
// over the 64-bit key hashes of the active lanes; sets S.flag (cleared by thread 0 when the node was popped), and the
// caller then commits the successors one at a time, in order.
template <int BLOCK, class SM>
__device__ __forceinline__ void dup_probe(SM &S, bool act, unsigned long long h64, int tid) {
  S.dupset[tid] = 0;
  S.dupset[tid + BLOCK] = 0;
  __syncthreads();
  if (act) {
    const unsigned long long hv = h64 | 1ull;
    uint32_t sl = (uint32_t)(h64 >> 7) & (2 * BLOCK - 1);
    for (;;) {
      unsigned long long old = atomicCAS(&S.dupset[sl], 0ull, hv);
      if (old == 0ull) break;
      if (old == hv) { S.flag = 1; break; }
      sl = (sl + 1) & (2 * BLOCK - 1);
    }
  }
  __syncthreads();
}

// ---- 5. termination tests behind an expansion (block-wide, one barrier), in the order of the reference loop: goal or
// t_max, then max_expand (an empty OPEN shows at the next pop); then the launch guard's heartbeat and the host's abort
// word, every 64th expansion.  is_goal(state): the kernel's goal predicate, evaluated by thread 0 on the expanded state
// (S.cur[0]).  True when the query has ended.
template <int BLOCK, int CONTROL, class SM, class Goal>
__device__ __forceinline__ bool search_ended(const QView<BLOCK, CONTROL, SM> &Q, int q, int tid, Goal is_goal) {
  const SearchParams &P = Q.P;
  SM &S = Q.S;
  if (tid == 0) {
    State s;
    for (int i = 0; i < 12; i++) ((double *)&s)[i] = S.cur[0][i];
    if (S.cur[0][12] >= P.t_max || is_goal(s))
      S.status = 0;
    else if (P.max_expand > 0 && S.c_expanded >= (unsigned long long)P.max_expand)
      S.status = 3;
    else if ((S.c_expanded & 63ull) == 0ull) {
      guard_mark(P, GUARD_BATCH, (uint32_t)q, S.c_expanded, (unsigned long long)S.n_nodes);
      if (guard_abort(P)) S.status = PLAN_ABORTED;
    }
  }
  __syncthreads();
  return S.status >= 0;
}

struct SpecCounts {  // QueryOut::spec; all zero for a kernel that expands one node per iteration (nothing speculative)
  unsigned long long v[4];
};

// ---- 6. recoverTraj and the result record (thread 0).  goal_id: the node the search ended on, NIL when the start was
// refused or already satisfied the goal.  edge_cost(parent id, action word of the predecessor record): the cost of
// that edge; spec: the speculation counters of QueryOut; load: how a state double is read back.
template <int EX, int BLOCK, int CONTROL, class SM, class EdgeCost, class Load = PlainLoad>
__device__ __forceinline__ void query_report(const QView<BLOCK, CONTROL, SM> &Q, int q, uint32_t goal_id, EdgeCost edge_cost, SpecCounts spec, unsigned long long t_begin,
                                             Load load = Load()) {
  using V = QView<BLOCK, CONTROL, SM>;
  const SearchParams &P = Q.P;
  SM &S = Q.S;
  constexpr int ns = key_len_c(CONTROL);
  QueryOut &o = P.out[q];
  int32_t *tn = P.traj_nodes + (size_t)q * (MAX_TRAJ + 1);
  int32_t *ta = P.traj_actions + (size_t)q * MAX_TRAJ;
  double *ts = P.traj_states + (size_t)q * (MAX_TRAJ + 1) * 13;
  int status = S.status;
  double cost = INFINITY;
  int len = 0;
  if (status == 0 && goal_id == NIL) {
    cost = S.tmp_d0;  // start already satisfied the goal
  } else if (status == 0) {
    // walk predecessor records: minimise g(pred) + edge cost, ties -> larger g(pred), then the
    // oldest record.  Written goal -> start; the host reverses.
    uint32_t node = goal_id;
    tn[0] = (int32_t)node;
    bool ok = true, too_long = false;
    while (V::pred(Q.node(node)) != NIL) {
      uint32_t best = NIL;
      double min_rhs = INFINITY, min_g = INFINITY;
      uint32_t hops = 0;
      for (uint32_t e = V::pred(Q.node(node)); e != NIL && hops <= S.n_edges; e = Q.edge(e)->next, hops++) {
        const EdgeRec er = *Q.edge(e);
        const double gp = V::g(Q.node(er.parent));
        const double rhs = gp + edge_cost(er.parent, er.action);
        if (rhs < min_rhs || (rhs == min_rhs && gp >= min_g)) { min_rhs = rhs; min_g = gp; best = e; }
      }
      if (best == NIL) { ok = false; break; }
      if (len >= MAX_TRAJ) { too_long = true; break; }
      ta[len] = (int32_t)(Q.edge(best)->action & EDGE_ACTION_MASK);
      node = Q.edge(best)->parent;
      len++;
      tn[len] = (int32_t)node;
      if (node == 0u) break;
    }
    if (too_long) {  // goal reached and cost known; the path does not fit the device-side buffer
      cost = V::g(Q.node(goal_id));
      status = 6;    // MPLX_PLAN_TRAJ_TOO_LONG
      len = 0;
    } else if (ok) {
      cost = V::g(Q.node(goal_id));
      for (int i = 0; i <= len; i++) {
        const double *st = V::state(Q.node((uint32_t)tn[i]));
        for (int k = 0; k < 12; k++) ts[i * 13 + k] = k < ns ? load(&st[k]) : 0.0;
        ts[i * 13 + 12] = load(&st[ns + EX]);
        if (EX && P.traj_yaw) P.traj_yaw[(size_t)q * (MAX_TRAJ + 1) + i] = st[ns];
      }
    } else {
      status = 1;
      len = 0;
    }
  }
  o.status = status;
  o.traj_len = len;
  o.cost = cost;
  o.n_expanded = S.c_expanded; o.n_closed = S.c_closed; o.n_nodes = S.n_nodes; o.n_edges = S.n_edges;
  o.n_primitives = S.c_prims; o.n_succ = S.c_succ; o.n_succ_finite = S.c_succ_finite; o.voxel_reads = S.c_reads;
  o.n_push = S.c_push; o.n_reopen = S.c_reopen; o.n_refill = S.c_refill; o.n_evict = S.c_evict;
  o.expand_hash = S.c_hash;
  o.n_recorded = (uint32_t)(S.c_expanded < P.cap_rec ? S.c_expanded : P.cap_rec);
  o.slot = blockIdx.x;
  for (int i = 0; i < 4; i++) o.spec[i] = spec.v[i];
  o.t_begin = t_begin;
  o.t_end = wall_clock64();
  for (int i = 0; i < 10; i++) o.cyc[i] = S.cyc[i];
}

// the query's node and predecessor chunk tables, for the host's state-space getters (block-wide, no barrier).
// keep = false: the chunks have gone back to the pools (a recycling launch keeps no state space: the host refuses them)
template <int BLOCK, int CONTROL, class SM>
__device__ __forceinline__ void publish_chunk_tables(const QView<BLOCK, CONTROL, SM> &Q, int q, int tid, bool keep = true) {
  const SearchParams &P = Q.P;
  for (uint32_t i = tid; i < (uint32_t)MAX_NODE_CH; i += BLOCK)
    P.node_tables[(size_t)q * MAX_NODE_CH + i] = (i < Q.S.node_chunks && keep) ? Q.node_chunk(i) : NIL;
  for (uint32_t i = tid; i < (uint32_t)MAX_EDGE_CH; i += BLOCK)
    P.edge_tables[(size_t)q * MAX_EDGE_CH + i] = (i < Q.S.edge_chunks && keep) ? Q.edge_chunk(i) : NIL;
}

}  // namespace mplx
