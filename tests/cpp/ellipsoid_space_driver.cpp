// getValidPrimitives / getAllPrimitives of MPL::EllipsoidPlanner (the mplx shim of ellipsoid_planner.h), served from the device's
// state-space export: the planning calls of mpl_test_node/src/ellipsoid_planner_node.cpp:64-175 as tests/cpp/ellipsoid_planner_driver.cpp
// makes them, then both getters.
// usage: ellipsoid_space_driver <cloud.bin: n x 3 doubles> n robot_r ox oy oz rx ry rz sx sy sz gx gy gz
//                               dt v_max a_max u_max u_max_z num w epsilon max_num use_3d use_jrk
// Prints one JSON line: the number of primitives each getter returned before and after plan(), and an FNV-1a digest (64 bit, over the
// bytes of the 18 coefficients of every primitive, axis by axis, in list order) of each list, which tests/test_cloud_space_shim.py
// compares with the Python path; exit code 3 when the device is missing (the counts are printed all the same).
#include <mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h>

#include <cstdlib>
#include <cstring>
#include <fstream>

static unsigned long long digest(const vec_E<Primitive<3>> &prs) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (const auto &pr : prs)
    for (int k = 0; k < 3; k++) {
      const Vec6f c = pr.pr(k).coeff();
      for (int j = 0; j < 6; j++) {
        const double v = c(j);
        unsigned char b[sizeof(double)];
        memcpy(b, &v, sizeof(double));
        for (size_t i = 0; i < sizeof(double); i++) h = (h ^ b[i]) * 0x100000001b3ull;
      }
    }
  return h;
}

int main(int argc, char **argv) {
  if (argc < 27) { printf("usage\n"); return 2; }
  const int n = atoi(argv[2]);
  std::vector<double> raw((size_t)n * 3);
  std::ifstream f(argv[1], std::ios::binary);
  f.read((char *)raw.data(), raw.size() * sizeof(double));
  vec_Vec3f map;
  for (int i = 0; i < n; i++) map.push_back(Vec3f(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]));
  const double robot_radius = atof(argv[3]);
  const Vec3f origin(atof(argv[4]), atof(argv[5]), atof(argv[6])), dim(atof(argv[7]), atof(argv[8]), atof(argv[9]));
  const double start_x = atof(argv[10]), start_y = atof(argv[11]), start_z = atof(argv[12]);
  const double goal_x = atof(argv[13]), goal_y = atof(argv[14]), goal_z = atof(argv[15]);
  const double dt = atof(argv[16]), v_max = atof(argv[17]), a_max = atof(argv[18]), u_max = atof(argv[19]), u_max_z = atof(argv[20]);
  const int num = atoi(argv[21]);
  const double w = atof(argv[22]), epsilon = atof(argv[23]);
  const int max_num = atoi(argv[24]);
  const bool use_3d = atoi(argv[25]) != 0, use_jrk = atoi(argv[26]) != 0, use_acc = true;

  std::unique_ptr<MPL::EllipsoidPlanner> planner_;
  planner_.reset(new MPL::EllipsoidPlanner(true));
  const MPL::PlannerBase<3, Waypoint3D> *base = planner_.get();  // (the getters are virtual: reached through the base as well)
  const size_t before_valid = base->getValidPrimitives().size(), before_all = base->getAllPrimitives().size();
  planner_->setMap(map, robot_radius, origin, dim);
  planner_->setEpsilon(epsilon);
  planner_->setVmax(v_max);
  planner_->setAmax(a_max);
  planner_->setDt(dt);
  planner_->setW(w);
  planner_->setMaxNum(max_num);
  planner_->setTol(2.0, 2.0, 100.0);

  Waypoint3D start;
  start.pos = Vec3f(start_x, start_y, start_z);
  start.vel = Vec3f(0, 0, 0);
  start.acc = Vec3f(0, 0, 0);
  start.jrk = Vec3f(0, 0, 0);
  start.use_pos = true;
  start.use_vel = true;
  start.use_acc = use_acc;
  start.use_jrk = use_jrk;
  start.use_yaw = false;
  Waypoint3D goal(start.control);
  goal.pos = Vec3f(goal_x, goal_y, goal_z);
  goal.vel = Vec3f(0, 0, 0);
  goal.acc = Vec3f(0, 0, 0);
  goal.jrk = Vec3f(0, 0, 0);

  vec_E<VecDf> U;
  const decimal_t du = u_max / num;
  if (use_3d) {
    decimal_t du_z = u_max_z / num;
    for (decimal_t dx = -u_max; dx <= u_max; dx += du)
      for (decimal_t dy = -u_max; dy <= u_max; dy += du)
        for (decimal_t dz = -u_max_z; dz <= u_max_z; dz += du_z) U.push_back(Vec3f(dx, dy, dz));
  } else {
    for (decimal_t dx = -u_max; dx <= u_max; dx += du)
      for (decimal_t dy = -u_max; dy <= u_max; dy += du) U.push_back(Vec3f(dx, dy, 0));
  }
  planner_->setU(U);

  const bool valid = planner_->plan(start, goal);
  const mplx_result &r = planner_->getResult();
  const bool ran = valid || r.n_expanded != 0 || r.status != 0;  // (false: the device or the map is missing)
  // a later change of the lattice or of dt must not change the primitives of the plan that was made
  planner_->setDt(2 * dt);
  planner_->setU(vec_E<VecDf>(1, Vec3f(0, 0, 0)));
  const vec_E<Primitive<3>> prs_valid = base->getValidPrimitives();
  const vec_E<Primitive<3>> prs_all = base->getAllPrimitives();
  printf("{\"ran\": %s, \"valid\": %s, \"status\": %d, \"n_nodes\": %llu, \"n_edges\": %llu, \"before_valid\": %zu, \"before_all\": %zu, "
         "\"valid_primitives\": %zu, \"all_primitives\": %zu, \"valid_digest\": \"%016llx\", \"all_digest\": \"%016llx\", \"t\": %.17g}\n",
         ran ? "true" : "false", valid ? "true" : "false", r.status, (unsigned long long)r.n_nodes, (unsigned long long)r.n_edges, before_valid,
         before_all, prs_valid.size(), prs_all.size(), digest(prs_valid), digest(prs_all), prs_valid.empty() ? 0.0 : prs_valid[0].t());
  return ran ? 0 : 3;
}
