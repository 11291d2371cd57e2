// tests/cpp/poly3_scene.h -- the 3-D moving-obstacle scene both 3-D planner drivers plan (tests/test_poly_map3d_shim.py builds
// the same scene in Python: SCENE there).  A 10 m x 10 m x 4 m box, a static box and a tilted static octahedron, a linear box
// (cov_v 0.1) and a box on an ACC trajectory; ACC control, the 27-input lattice of u = 1, dt 0.5, v_max 2, a_max 1.5, w 10.
#pragma once
#include <vector>

namespace poly3_scene {
const double ORI[3] = {0.0, -5.0, 0.0}, DIM[3] = {10.0, 10.0, 4.0}, START_T = 0.5;
const double DT = 0.5, V_MAX = 2.0, A_MAX = 1.5, J_MAX = -1.0, W = 10.0, EPS = 1.0, TOL_POS = 0.5;
const int MAX_NUM = 3000;
const double START[3] = {1.0, 0.0, 2.0}, GOAL[3] = {6.5, 1.0, 3.5};  // (over the static box; the dynamics-aware heuristic)
const double S3 = 0.5773502691896258;  // 1 / sqrt(3)
inline std::vector<double> box(double h) {  // rows {px, py, pz, nx, ny, nz}
  return {-h, 0, 0, -1, -0.0, -0.0, h, 0, 0, 1, 0, 0, 0, -h, 0, -0.0, -1, -0.0, 0, h, 0, 0, 1, 0, 0, 0, -h, -0.0, -0.0, -1, 0, 0, h, 0, 0, 1};
}
inline std::vector<double> octahedron(double r) {
  std::vector<double> v;
  for (int sx = -1; sx <= 1; sx += 2)
    for (int sy = -1; sy <= 1; sy += 2)
      for (int sz = -1; sz <= 1; sz += 2) {
        const double row[6] = {sx * r, 0.0, 0.0, sx * S3, sy * S3, sz * S3};
        v.insert(v.end(), row, row + 6);
      }
  return v;
}
const double STATIC_P[2][3] = {{4.5, 0.5, 2.0}, {6.5, -2.0, 1.5}};
const double LIN_P[3] = {6.0, 3.0, 2.0}, LIN_V[3] = {0.0, -0.5, 0.0}, LIN_COV = 0.1;
// the ACC trajectory: from (3, -3, 2) at rest, inputs (0, 1, 0) twice then (0, 0, 0) twice, dt 0.5: rows {cx[6], cy[6], cz[6], T}
inline std::vector<double> nl_segs() {
  double p[3] = {3.0, -3.0, 2.0}, v[3] = {0, 0, 0};
  const double us[4][3] = {{0, 1, 0}, {0, 1, 0}, {0, 0, 0}, {0, 0, 0}};
  std::vector<double> s;
  for (int i = 0; i < 4; i++) {
    for (int k = 0; k < 3; k++) {
      const double row[6] = {0, 0, 0, us[i][k], v[k], p[k]};
      s.insert(s.end(), row, row + 6);
    }
    s.push_back(DT);
    for (int k = 0; k < 3; k++) {
      p[k] = us[i][k] / 2 * DT * DT + v[k] * DT + p[k];
      v[k] = us[i][k] * DT + v[k];
    }
  }
  return s;
}
const double NL_START_T = 0.3;
inline std::vector<double> lattice() {  // x, y, z from -1 to 1 in steps of 1, the loop variable accumulating the step
  std::vector<double> U;
  for (double x = -1.0; x <= 1.0; x += 1.0)
    for (double y = -1.0; y <= 1.0; y += 1.0)
      for (double z = -1.0; z <= 1.0; z += 1.0) { U.push_back(x); U.push_back(y); U.push_back(z); }
  return U;
}
}  // namespace poly3_scene
