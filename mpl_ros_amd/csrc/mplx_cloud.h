// mplx_cloud.h -- the point-cloud environment (env_cloud + EllipsoidUtil of the ellipsoid planner) on the device:
//   * a bucketed index of the cloud built on the device (cloud_index_key_kernel / cloud_index_scan_kernel / cloud_index_scatter_kernel),
//   * env_cloud::get_succ for K states (cloud_get_succ_kernel: the parity entry),
//   * astar_cloud_kernel: GraphSearch::Astar over env_cloud, one workgroup per query, on the search machinery of
//     mplx_kernels.h (Smem, OPEN structure, pools, hash table, commit_parallel) and the per-query steps of mplx_search_steps.h,
//   * astar_cloud_prior_kernel: the same search with the heuristic guided by a prior trajectory (the P-list below).
//
// Index.  Points are bucketed by the cell of edge L = 1.0625 r_f (r_f = (float)r) they fall in; the cell's three integer
// coordinates are hashed to one of M = next_pow2(n) buckets and the points are counting-sorted by bucket (count, scan,
// scatter): start[M + 1] offsets, then the points in bucket order, once as float xyz (the radius filter) and once as
// double xyz (the ellipsoid test).  Memory is O(n) whatever the cloud's extent: cells that share a bucket are simply
// visited together (the float filter drops the strangers).  The order of the points inside a bucket is not fixed (the
// scatter uses atomics); no decision depends on it.
//
// Why visiting the 27 cells around a sample's cell is conservative.  Cell coordinates are u = floor((double)x_f * inv_L)
// of the FLOAT coordinate x_f, for points and sample centres alike, clamped to +-2^40.  A point the float filter accepts
// has a computed squared distance below fl((double)r_f * r_f); the float rounding of three differences, three squares and
// two sums moves that by less than 8 ulp, so each true coordinate difference |x_f - c_f| < r_f (1 + 2^-20).  The double
// products x_f * inv_L carry a relative error below 2^-52, i.e. an absolute error below 2^-12 cell for |u| < 2^40.  So
// |u_point - u_centre| < (1 + 2^-20) / 1.0625 + 2^-11 < 1, and their floors differ by at most one.  Coordinates clamped
// at +-2^40 cells (beyond 5e11 r) fall into the same extreme cell as a centre clamped the same way; a point clamped on an
// axis where the centre is not is farther than r from it and cannot pass the filter.
//
// E-LIST -- the evaluation order both this file and the CPU checker (tests/cloud_checker.py) follow.  The reference's
// own sources for PCL/FLANN and DecompUtil are not in the tree; E2, E3 and E5 restate recollections of them.
//   E1  bounding box: pr.sample(2) = evaluate(i * (dt / 2)), i = 0, 1, 2; each position must pass Polyhedron3D::inside
//       with the six planes of setBoundingBox (third point ori + (dim.x / 2, dim.z / 2, 0) included): for every plane
//       (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2) <= 1e-10.  Every obstacle point is kept (setObstacles runs
//       before setBoundingBox, when the box has no planes).
//   E2  radius filter [UNVERIFIED recollection of PCL KdTreeFLANN + flann::L2_Simple<float>]: centre c_f = (float)d,
//       point p_f = (float)p, dx = p_f.x - c_f.x (float), dist = (dx dx + dy dy) + dz dz (float), candidate iff
//       dist < (float)((double)r_f * r_f).
//   E3  ellipsoid test [UNVERIFIED recollection of DecompUtil Ellipsoid3D::inside]: v = p - d (double), y = C^-1 v with
//       y_i = (Ci(i,0) v0 + Ci(i,1) v1) + Ci(i,2) v2, inside iff sqrt((y0 y0 + y1 y1) + y2 y2) <= 1.
//   E4  C^-1 is Eigen's 3x3 cofactor inverse: cof(i,j) = m(i1,j1) m(i2,j2) - m(i1,j2) m(i2,j1) (i1 = i+1 mod 3, ...),
//       det = (cof(0,0) m00 + cof(1,0) m10) + cof(2,0) m20, invdet = 1 / det, Ci(i,j) = cof(j,i) * invdet.
//   E5  ellipsoid of a sample (pos, acc): e = (acc0 + 0, acc1 + 0, acc2 + 9.81); normalize(v) = v / sqrt((x x + y y) + z z);
//       b3 = normalize(e), b2 = normalize(b3 x (1, 0, 0)), b1 = normalize(b2 x b3), cross products written out in full
//       (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); R = [b1 b2 b3]; M = R diag(r, r, 0.1) and C = M R^T, every
//       matrix product coefficient summed as (x0 y0 + x1 y1) + x2 y2 over all three terms, zeros included.
//   E6  samples: max_v = max over axes of max_vel (the same as the voxel path: validate_and_maxv_c), n = ceil(max_v dt / r),
//       ellipsoid j = 0..n at t = j * (dt / n).  n = 0 tests only t = 0 (as D4); it cannot happen after the tn == curr test.
//   E7  empty cloud: every primitive passes the point test (the reference's PCL refuses an empty cloud).
//   E8  get_succ skips a primitive when tn == curr (same state key), when validate_primitive fails or when isFree fails
//       (E1, then E2-E6): no infinite-cost successors, n_succ == n_succ_finite.  Cost J(control) + w dt.  The start is
//       always free (env_cloud::is_free returns true).  Expanded nodes are not recorded (env_cloud.h:57 is commented out).
//   E9  points that are not finite: a point with a NaN or infinite coordinate, or one whose float coordinate overflows
//       (1e300) or whose squared float distance does (1e30), fails dist < r2f in E2, so it blocks nothing and changes
//       no other decision; its cell coordinate is clamped (NaN to -2^40).  This project's choice: what PCL does with
//       such a cloud is not known here.
//
// P-LIST -- a search guided by a prior trajectory (PlannerBase::setPriorTrajectory, ellipsoid_planner_node.cpp:121-139),
// followed by the kernel, the shim, the Python front end and the CPU checker (tests/cloud_prior_checker.py).  P1 and P2
// restate recollections of the un-vendored MPL v1.2.
//   P1  sampling [UNVERIFIED recollection of env_base::set_prior_trajectory] (host code: the shim and
//       ellipsoid.prior_from_traj): prior.clear(); T = traj.getTotalTime(); for (t = 0; t < T; t += dt) prior.push_back(
//       {traj.evaluate(t), w (T - t)}), with the dt and w in force at the call and t accumulated by repeated f64
//       addition.  An entry's control kind is the low four bits of the evaluated waypoint's control.
//   P2  get_heur(state) [UNVERIFIED recollection of env_base::get_heur]: 0 when the state's key equals the goal's; else,
//       with a prior of n entries, t = state.t >= 0 and id = (uint64)(t / dt) < n:
//       cal_heur(state -> prior[id].state, target control prior[id].control) + prior[id].cost_to_go; else
//       cal_heur(state -> goal).  A negative or NaN t takes the goal branch; so does a quotient at or past n, however large
//       (the comparison is made on the f64 quotient: floor(x) < n iff x < n for x >= 0).  heur_ignore_dynamics applies
//       to cal_heur as ever, on the target's position; eps == 0 gives 0.
//   P3  time is no part of the key: a state's h is computed once, when the state is created, from the time of the arrival
//       that creates it (the first arrival in sequential A* order, which is the order the commit creates states in).
//       All successors of one expansion share t = t(expanded) + dt, so they share the prior entry.
//   P4  the start's h uses start.t: the prior is indexed by absolute state time.
//   P5  the goal test, t_max, costs, the (f, g, id) order, D6 and recoverTraj are unchanged.  A prior makes the heuristic
//       inconsistent in general: re-opened states and popped f values below the current bucket are ordinary here.
// The table of a query (12 state doubles, control kind and cost-to-go per entry) is staged in LDS at query start when it
// has at most CLOUD_PRIOR_LDS_CAP entries and is read from global memory otherwise; the heuristic reads it through
// one generic pointer either way, so both paths run the same arithmetic.
#pragma once
#include "mplx_kernels.h"

namespace mplx {

constexpr double CLOUD_CELL_MARGIN = 1.0625;  // cell edge / r_f
constexpr double CLOUD_U_CLAMP = 1099511627776.0;  // 2^40 cells
constexpr double CLOUD_BBOX_EPS = 1e-10;

struct CloudDev {
  const float4 *pf;       // n points in bucket order: float xyz (w unused)
  const double *pd;       // the same points: double xyz
  const uint32_t *start;  // bucket_mask + 2 offsets
  uint32_t n_pts, bucket_mask;
  double inv_cell;        // 1 / (1.0625 r_f)
  float r2f;              // (float)((double)r_f * r_f)
  float pad;
  double axe[3];          // (r, r, 0.1)
  double bq[6][3], bn[6][3];  // bounding-box planes: point, normal (setBoundingBox)
};

__device__ __forceinline__ long long cloud_cell_1(float x, double inv_cell) {
  double u = floor((double)x * inv_cell);
  u = fmin(fmax(u, -CLOUD_U_CLAMP), CLOUD_U_CLAMP);  // (NaN: fmax returns the bound)
  return (long long)u;
}
__device__ __forceinline__ uint32_t cloud_bucket(long long ix, long long iy, long long iz, uint32_t mask) {
  unsigned long long h = (unsigned long long)ix * 0x9E3779B97F4A7C15ull ^ (unsigned long long)iy * 0xC2B2AE3D27D4EB4Full ^ (unsigned long long)iz * 0x165667B19E3779F9ull;
  h ^= h >> 31;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 29;
  return (uint32_t)h & mask;
}

// ---- index build: key + count, scan, scatter (plain kernels: one translation unit only, mplx_cloud.hip)
#ifndef MPLX_CLOUD_SEARCH_ONLY
__global__ void cloud_index_key_kernel(uint32_t n, const double *__restrict__ pts, double inv_cell, uint32_t mask, uint32_t *__restrict__ bucket, uint32_t *__restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = (float)pts[3 * (size_t)i], y = (float)pts[3 * (size_t)i + 1], z = (float)pts[3 * (size_t)i + 2];
  const uint32_t b = cloud_bucket(cloud_cell_1(x, inv_cell), cloud_cell_1(y, inv_cell), cloud_cell_1(z, inv_cell), mask);
  bucket[i] = b;
  atomicAdd(&count[b], 1u);
}
// exclusive scan of m counts into start[0..m] by one workgroup of 1024 threads (each a contiguous slice)
__global__ __launch_bounds__(1024) void cloud_index_scan_kernel(const uint32_t *__restrict__ count, uint32_t m, uint32_t *__restrict__ start) {
  __shared__ uint32_t part[1024];
  const uint32_t tid = threadIdx.x, per = (m + 1023u) / 1024u, lo = tid * per < m ? tid * per : m, hi = lo + per < m ? lo + per : m;
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += count[i];
  part[tid] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - s;
  for (uint32_t i = lo; i < hi; i++) {
    start[i] = run;
    run += count[i];
  }
  if (tid == 1023u) start[m] = part[1023];
}
__global__ void cloud_index_scatter_kernel(uint32_t n, const double *__restrict__ pts, const uint32_t *__restrict__ bucket, const uint32_t *__restrict__ start, uint32_t *__restrict__ cursor,
                                     float4 *__restrict__ pf, double *__restrict__ pd) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = bucket[i];
  const uint32_t at = start[b] + atomicAdd(&cursor[b], 1u);
  const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  pf[at] = make_float4((float)x, (float)y, (float)z, 0.0f);
  pd[3 * (size_t)at] = x; pd[3 * (size_t)at + 1] = y; pd[3 * (size_t)at + 2] = z;
}

#endif  // MPLX_CLOUD_SEARCH_ONLY

// ---- geometry (E1, E4, E5)
__device__ __forceinline__ bool cloud_in_bbox(const CloudDev &C, double x, double y, double z) {
  bool in = true;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double s = (C.bn[k][0] * (x - C.bq[k][0]) + C.bn[k][1] * (y - C.bq[k][1])) + C.bn[k][2] * (z - C.bq[k][2]);
    in = in && !(s > CLOUD_BBOX_EPS);
  }
  return in;
}
__device__ __forceinline__ void cloud_normalize(double *v) {
  const double z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];  // (Eigen's normalized(): unchanged when the norm is 0)
  if (z > 0.0) {
    const double s = sqrt(z);
    v[0] = v[0] / s; v[1] = v[1] / s; v[2] = v[2] / s;
  }
}
__device__ __forceinline__ void cloud_cross(const double *a, const double *b, double *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// C^-1 (row-major) of the ellipsoid at a sample with acceleration acc (E4, E5)
__device__ __forceinline__ void cloud_ellipsoid_inv(const double *axe, const double *acc, double *ci) {
  double b3[3] = {acc[0] + 0.0, acc[1] + 0.0, acc[2] + 9.81};
  cloud_normalize(b3);
  const double bc[3] = {1.0, 0.0, 0.0};
  double b2[3], b1[3];
  cloud_cross(b3, bc, b2);
  cloud_normalize(b2);
  cloud_cross(b2, b3, b1);
  cloud_normalize(b1);
  double R[3][3], D[3][3] = {{axe[0], 0.0, 0.0}, {0.0, axe[1], 0.0}, {0.0, 0.0, axe[2]}}, M[3][3], m[3][3];
  for (int i = 0; i < 3; i++) { R[i][0] = b1[i]; R[i][1] = b2[i]; R[i][2] = b3[i]; }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[i][j] = (R[i][0] * D[0][j] + R[i][1] * D[1][j]) + R[i][2] * D[2][j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m[i][j] = (M[i][0] * R[j][0] + M[i][1] * R[j][1]) + M[i][2] * R[j][2];
  double cof[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    }
  const double det = (cof[0][0] * m[0][0] + cof[1][0] * m[1][0]) + cof[2][0] * m[2][0];
  const double invdet = 1.0 / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) ci[3 * i + j] = cof[j][i] * invdet;
}
__device__ __forceinline__ bool cloud_inside(const double *ci, const double *d, double px, double py, double pz) {
  const double v0 = px - d[0], v1 = py - d[1], v2 = pz - d[2];
  const double y0 = (ci[0] * v0 + ci[1] * v1) + ci[2] * v2;
  const double y1 = (ci[3] * v0 + ci[4] * v1) + ci[5] * v2;
  const double y2 = (ci[6] * v0 + ci[7] * v1) + ci[8] * v2;
  return sqrt((y0 * y0 + y1 * y1) + y2 * y2) <= 1.0;
}

// ---- one expansion: env_cloud::get_succ of S.cur[0]
template <int BLOCK>
struct CloudLds {
  int32_t nsmp[BLOCK];    // n of the lane's primitive (E6), -1: skipped before the point test
  int32_t hit[BLOCK];     // an obstacle point is inside one of the primitive's ellipsoids
  uint32_t offs[BLOCK + 1];
  double ed[BLOCK][3];    // the chunk's ellipsoids: centre, C^-1, float centre, primitive
  double eci[BLOCK][9];
  float ef[BLOCK][3];
  int32_t ep[BLOCK];
  uint32_t tests;         // points the radius filter looked at in this expansion
};

// Lane i < n_u builds primitive i (the voxel path's prim_build_axis / evaluate / key / validate_and_maxv_c) and the
// bounding-box test; the (primitive, ellipsoid sample) pairs are flattened over the workgroup in chunks of BLOCK, each
// lane stages one ellipsoid in LDS, then the (pair, neighbour cell) work items are spread over all lanes, each walking the
// points of one bucket; a primitive stops being looked at once one of its ellipsoids holds a point.
template <int BLOCK, int CONTROL, class SM>
__device__ __forceinline__ void cloud_expand(const SearchParams &P, const CloudDev &C, SM &S, CloudLds<BLOCK> &E, int tid, LaneSucc &L) {
  const double T = P.dt;
  L.valid = false;
  L.blocked = false;
  L.reads = 0;
  int ns = -1;
  if (tid < P.n_u) {
    double c[3][6];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) prim_build_axis(CONTROL, S.cur[0][ax], S.cur[0][3 + ax], S.cur[0][6 + ax], S.cur[0][9 + ax], lane_u(S, P, tid, ax, 0), c[ax]);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      L.tn.p[ax] = pos_at_c<CONTROL>(c[ax], T);
      L.tn.v[ax] = vel_at_c<CONTROL>(c[ax], T);
      L.tn.a[ax] = acc_at_c<CONTROL>(c[ax], T);
      L.tn.j[ax] = jrk_at_c<CONTROL>(c[ax], T);
    }
    state_key_c<CONTROL>(L.tn, L.key);
    uint32_t kdiff = 0;
#pragma unroll
    for (int i = 0; i < key_len_c(CONTROL); i++) kdiff |= (uint32_t)(L.key[i] ^ S.cur_key[0][i]);
    double max_v = 0.0;
    bool ok = kdiff != 0u && validate_and_maxv_c<CONTROL>(c, T, P.v_max, P.a_max, P.j_max, &max_v);
    if (ok) {  // E1
      const double h = T / 2;
      for (int i = 0; i <= 2 && ok; i++) {
        const double t = (double)i * h;
        ok = cloud_in_bbox(C, pos_at_c<CONTROL>(c[0], t), pos_at_c<CONTROL>(c[1], t), pos_at_c<CONTROL>(c[2], t));
      }
    }
    if (ok) ns = (int)ceil(max_v * T / C.axe[0]);
    E.nsmp[tid] = ns;
    E.hit[tid] = 0;
  }
  if (tid == 0) E.tests = 0;
  uint32_t total;
  const uint32_t off = block_excl_scan<BLOCK>(ns >= 0 && C.n_pts > 0 ? (uint32_t)ns + 1u : 0u, S, tid, total);  // (E7: nothing to test)
  if (tid < P.n_u) E.offs[tid] = off;
  if (tid == 0) E.offs[P.n_u] = total;
  __syncthreads();
  volatile int32_t *hitv = E.hit;
  uint32_t tests = 0;
  for (uint32_t base = 0; base < total; base += BLOCK) {
    const uint32_t e = base + (uint32_t)tid;
    if (e < total) {
      int lo = 0, hi = P.n_u;  // largest p with offs[p] <= e
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (E.offs[mid] <= e) lo = mid; else hi = mid;
      }
      const int p = lo;
      const int n = E.nsmp[p];
      if (hitv[p]) {
        E.ep[tid] = -1;
      } else {
        const uint32_t j = e - E.offs[p];
        const double t = n == 0 ? 0.0 : (double)j * (T / n);  // (E6)
        double c[3][6], d[3], acc[3];
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
          prim_build_axis(CONTROL, S.cur[0][ax], S.cur[0][3 + ax], S.cur[0][6 + ax], S.cur[0][9 + ax], lane_u(S, P, p, ax, 0), c[ax]);
          d[ax] = pos_at_c<CONTROL>(c[ax], t);
          acc[ax] = acc_at_c<CONTROL>(c[ax], t);
        }
        double ci[9];
        cloud_ellipsoid_inv(C.axe, acc, ci);
        for (int k = 0; k < 3; k++) { E.ed[tid][k] = d[k]; E.ef[tid][k] = (float)d[k]; }
        for (int k = 0; k < 9; k++) E.eci[tid][k] = ci[k];
        E.ep[tid] = p;
      }
    }
    __syncthreads();
    const uint32_t np = total - base < (uint32_t)BLOCK ? total - base : (uint32_t)BLOCK;
    for (uint32_t k = tid; k < np * 27u; k += BLOCK) {
      const uint32_t pi = k / 27u, nb = k % 27u;
      const int p = E.ep[pi];
      if (p < 0 || hitv[p]) continue;
      const float cx = E.ef[pi][0], cy = E.ef[pi][1], cz = E.ef[pi][2];
      const long long ix = cloud_cell_1(cx, C.inv_cell) + (long long)(nb % 3u) - 1, iy = cloud_cell_1(cy, C.inv_cell) + (long long)((nb / 3u) % 3u) - 1,
                      iz = cloud_cell_1(cz, C.inv_cell) + (long long)(nb / 9u) - 1;
      const uint32_t b = cloud_bucket(ix, iy, iz, C.bucket_mask);
      const uint32_t q0 = C.start[b], q1 = C.start[b + 1];
      for (uint32_t q = q0; q < q1; q++) {
        if (((q - q0) & 15u) == 15u && hitv[p]) break;  // another lane has blocked this primitive
        const float4 pf = C.pf[q];
        tests++;
        const float dx = pf.x - cx, dy = pf.y - cy, dz = pf.z - cz;
        const float dist = (dx * dx + dy * dy) + dz * dz;  // (E2)
        if (!(dist < C.r2f)) continue;
        const double *pd = C.pd + 3 * (size_t)q;
        if (cloud_inside(E.eci[pi], E.ed[pi], pd[0], pd[1], pd[2])) {  // (E3)
          hitv[p] = 1;
          break;
        }
      }
    }
    __syncthreads();
  }
  if (tests) atomicAdd(&E.tests, tests);
  __syncthreads();
  if (tid < P.n_u) L.valid = ns >= 0 && !hitv[tid];
}

// One successor of env_cloud::get_succ (mirrors mplx_cloud_succ)
struct CloudSuccOut {
  double state[13];  // pos3 vel3 acc3 jrk3 t
  double cost;       // J(control) + w dt; +inf when the primitive is skipped
  int32_t action, valid;
};

template <int BLOCK, int CONTROL>
__global__ __launch_bounds__(BLOCK) void cloud_get_succ_kernel(SearchParams P, CloudDev C, int K, const double *states, CloudSuccOut *out, unsigned long long *tests) {
  __shared__ Smem<BLOCK> S;
  __shared__ CloudLds<BLOCK> E;
  const int tid = threadIdx.x;
  fill_uq<BLOCK, CONTROL>(P, S, tid);
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    if (tid < 13) S.cur[0][tid] = states[13 * (size_t)k + tid];
    __syncthreads();
    if (tid == 0) {
      State s;
      for (int i = 0; i < 12; i++) ((double *)&s)[i] = S.cur[0][i];
      state_key_c<CONTROL>(s, S.cur_key[0]);
    }
    __syncthreads();
    LaneSucc L;
    cloud_expand<BLOCK, CONTROL>(P, C, S, E, tid, L);
    if (tid < P.n_u) {
      CloudSuccOut &o = out[(size_t)k * P.n_u + tid];
      for (int ax = 0; ax < 3; ax++) {
        o.state[ax] = L.tn.p[ax];
        o.state[3 + ax] = L.tn.v[ax];
        o.state[6 + ax] = L.tn.a[ax];
        o.state[9 + ax] = L.tn.j[ax];
      }
      o.state[12] = S.cur[0][12] + P.dt;
      o.cost = L.valid ? S.ucost_lds[tid] : INFINITY;
      o.action = tid;
      o.valid = L.valid ? 1 : 0;
    }
    if (tid == 0) atomicAdd(tests, (unsigned long long)E.tests);
    __syncthreads();
  }
}

// ---- the prior trajectory of a search (P-list)
constexpr int CLOUD_PRIOR_LDS_CAP = 256;  // entries staged in LDS: 27 KB beside the search's 87 KB, one workgroup per CU either way

struct CloudPriorDev {
  const int32_t *begin;    // per query: its first entry
  const int32_t *count;    // per query: its entries (0: no prior)
  const double *state;     // 12 per entry: pos3 vel3 acc3 jrk3
  const double *ctg;       // cost-to-go w (T - t)
  const int32_t *control;  // control kind of the entry
};
struct CloudPriorLds {
  double state[CLOUD_PRIOR_LDS_CAP][12];
  double ctg[CLOUD_PRIOR_LDS_CAP];
  int32_t control[CLOUD_PRIOR_LDS_CAP];
};
// one query's table, in LDS or in global memory: generic pointers
struct CloudPriorView {
  const double *state, *ctg;
  const int32_t *control;
  uint32_t n;
};

// P2.  t: the state's time; dt: the planner's
__device__ __forceinline__ double cloud_prior_heur(const HeurParams &hp, int control, const State &s, const int32_t *key, int nkey, double t, double dt, const CloudPriorView &R) {
  if ((control & 15) == (hp.goal_control & 15) && nkey == hp.goal_nkey) {
    uint32_t diff = 0;
    for (int i = 0; i < nkey; i++) diff |= (uint32_t)(key[i] ^ hp.goal_key[i]);
    if (diff == 0u) return 0.0;
  }
  if (R.n > 0u && t >= 0.0) {
    const double x = t / dt;
    if (x < (double)R.n) {
      const uint32_t id = (uint32_t)x;
      State tg;
      const double *src = R.state + 12 * (size_t)id;
#pragma unroll
      for (int i = 0; i < 12; i++) ((double *)&tg)[i] = src[i];
      return cal_heur_to(hp.w, hp.v_max, hp.heur_ignore_dynamics, control, s, tg, R.control[id]) + R.ctg[id];
    }
  }
  return cal_heur(hp, control, s);
}

// ---- GraphSearch::Astar over env_cloud: the per-query steps of mplx_search_steps.h around cloud_expand; the start
// always free (E8), no yaw, no potential.  Keys: the voxel environment's (no time key); order (f, g, id) (D5);
// a closed state that improves is re-opened (D6).  PRIOR: the heuristic of the P-list, from the query's table in PR.
template <int BLOCK, int CONTROL, bool PRIOR>
__device__ __forceinline__ void astar_cloud_search(const SearchParams &P, const CloudDev &C, const CloudPriorDev &PR) {
  __shared__ Smem<BLOCK> S;
  __shared__ CloudLds<BLOCK> E;
  using V = QView<BLOCK, CONTROL>;
  const int tid = threadIdx.x;
  const V Q{P, S, P.bkt_head + (size_t)blockIdx.x * 2 * NB * NSUB};
  constexpr int nk = key_len_c(CONTROL);
  fill_uq<BLOCK, CONTROL>(P, S, tid);
  for (;;) {
    if (tid == 0) {
      S.q_index = atomicAdd(P.next_query, 1);
      if (guard_abort(P)) S.q_index = P.nq;
    }
    __syncthreads();
    const int qi = S.q_index;
    if (qi >= P.nq) break;
    const int q = P.order[qi];
    const QueryIn &in = P.queries[q];
    const unsigned long long t_begin = wall_clock64();
    query_reset(Q, in, (uint32_t)P.n_u, tid);
    CloudPriorView R{nullptr, nullptr, nullptr, 0u};
    if constexpr (PRIOR) {  // (the barrier behind the admission orders the staging stores before the first read)
      __shared__ CloudPriorLds PL;
      const uint32_t n = (uint32_t)PR.count[q];
      const size_t b = (size_t)PR.begin[q];
      if (n <= (uint32_t)CLOUD_PRIOR_LDS_CAP) {
        for (uint32_t i = tid; i < 12u * n; i += BLOCK) (&PL.state[0][0])[i] = PR.state[12 * b + i];
        for (uint32_t i = tid; i < n; i += BLOCK) {
          PL.ctg[i] = PR.ctg[b + i];
          PL.control[i] = PR.control[b + i];
        }
        R = CloudPriorView{&PL.state[0][0], PL.ctg, PL.control, n};
      } else {
        R = CloudPriorView{PR.state + 12 * b, PR.ctg + b, PR.control + b, n};
      }
    }
    if (tid == 0) query_admit(Q, in, true, is_goal_state(in.start, in.goal, in.goal_control, P.tol_pos, P.tol_vel, P.tol_acc));  // (E8: the start is always free)
    __syncthreads();
    uint32_t goal_id = NIL;
    if (S.status < 0) {
      const bool started = query_start<nk, 0>(Q, in, q, tid, 0, 0.0, [&](const int32_t *key) {
        if constexpr (PRIOR) return cloud_prior_heur(S.hp, CONTROL, in.start, key, nk, in.start_t, P.dt, R);  // (P4)
        else return get_heur(S.hp, CONTROL, in.start, key, nk);
      });
      if (started) for (;;) {
        while (S.n_near + S.reserve > (uint32_t)NC) {
          evict_half(Q, tid);
          __syncthreads();
        }
        const bool popped = pop_min<BLOCK, CONTROL, Smem<BLOCK>, nk, 0>(Q, tid);
        if (!popped) {
          if (tid == 0) S.status = 1;
          __syncthreads();
          break;
        }
        const uint32_t cur = S.cur_id;
        if (tid == 0) {
          S.c_expanded++;
          S.c_closed++;
          S.c_hash = S.c_hash * 0x100000001B3ull + (unsigned long long)(cur + 1u);
          if (P.rec_ids && S.c_expanded <= P.cap_rec) P.rec_ids[(size_t)q * P.cap_rec + (S.c_expanded - 1)] = (int32_t)cur;
          S.flag = 0;
        }
        LaneSucc L;
        cloud_expand<BLOCK, CONTROL>(P, C, S, E, tid, L);
        const bool act = L.valid;
        {
          uint32_t tot;
          block_excl_scan<BLOCK>(act ? 1u : 0u, S, tid, tot);
          if (tid == 0) {
            S.c_prims += (unsigned long long)P.n_u;
            S.c_succ += tot;
            S.c_succ_finite += tot;
            S.c_reads += E.tests;
          }
        }
        const unsigned long long h64 = act ? key_hash64(L.key, nk) : 0ull;
        dup_probe<BLOCK>(S, act, h64, tid);
        const double lane_cost = act ? S.ucost_lds[tid] : 0.0;
        if constexpr (PRIOR) {
          // (P3) the heuristic of a state this expansion creates: every successor arrives at t(expanded) + dt
          auto heur = [&](const LaneSucc &l) { return cloud_prior_heur(S.hp, CONTROL, l.tn, l.key, nk, S.cur[0][12] + P.dt, P.dt, R); };
          using H = decltype(heur);
          if (!S.flag) {
            commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, nk, false, NoCreateHook, H>(Q, tid, q, act, L, h64, lane_cost, (uint32_t)tid, false, 0, NoCreateHook(), heur);
          } else {
            for (int i = 0; i < P.n_u && S.status < 0; i++)
              commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, nk, false, NoCreateHook, H>(Q, tid, q, act && tid == i, L, h64, lane_cost, (uint32_t)tid, false, 0, NoCreateHook(), heur);
          }
        } else {
          if (!S.flag) {
            commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, nk, false>(Q, tid, q, act, L, h64, lane_cost, (uint32_t)tid);
          } else {
            for (int i = 0; i < P.n_u && S.status < 0; i++) commit_parallel<BLOCK, CONTROL, Smem<BLOCK>, nk, false>(Q, tid, q, act && tid == i, L, h64, lane_cost, (uint32_t)tid);
          }
        }
        __syncthreads();
        if (S.status >= 0) break;  // pool full
        if (search_ended(Q, q, tid, [&](const State &s) { return is_goal_state(s, S.hp.goal, S.hp.goal_control, P.tol_pos, P.tol_vel, P.tol_acc); })) break;
      }
      goal_id = S.cur_id;
      clear_buckets(Q, tid);
    }
    __syncthreads();
    if (tid == 0) query_report<0>(Q, q, goal_id, [&](uint32_t, uint32_t action) { return P.ucost[action & EDGE_ACTION_MASK]; }, SpecCounts{}, t_begin);
    publish_chunk_tables(Q, q, tid);
    __syncthreads();
  }
}

template <int BLOCK, int CONTROL>
__global__ __launch_bounds__(BLOCK) void astar_cloud_kernel(SearchParams P, CloudDev C) {
  astar_cloud_search<BLOCK, CONTROL, false>(P, C, CloudPriorDev{});
}
// the search guided by prior trajectories: instantiated in mplx_cloud_prior.hip only
template <int BLOCK, int CONTROL>
__global__ __launch_bounds__(BLOCK) void astar_cloud_prior_kernel(SearchParams P, CloudDev C, CloudPriorDev PR) {
  astar_cloud_search<BLOCK, CONTROL, true>(P, C, PR);
}

}  // namespace mplx

// mplx_cloud_prior.hip: the prior-aware search for P.control (false: no build for it), and P2 for K states
bool mplx_cloud_prior_launch(int grid, hipStream_t s, const mplx::SearchParams &P, const mplx::CloudDev &D, const mplx::CloudPriorDev &PR);
void mplx_cloud_heuristic_launch(hipStream_t s, int control, const mplx::HeurParams &hp, double dt, const mplx::CloudPriorView &R, int K, const double *states, double *h);
