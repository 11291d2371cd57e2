// The prior-trajectory flow of mpl_test_node/src/ellipsoid_planner_node.cpp:63-163 without ROS, against the mplx shim
// headers: setMap and the setters, a cheap plan in ACC states (use_pos, use_vel) standing in for the trajectory the node
// reads from a bag, setPriorTrajectory(that trajectory) after setDt and setW (:135), the goal's use_acc / use_jrk cleared
// (:136-137), then the plan in JRK states (use_pos, use_vel, use_acc) guided by the prior.
// usage: ellipsoid_prior_driver <cloud.bin: n x 3 doubles> n robot_r ox oy oz rx ry rz sx sy sz gx gy gz
//                               dt v_max a_max u_max u_max_z num w epsilon max_num use_3d
// Prints one JSON line: cost and expansion count of both plans and the guided trajectory (its waypoints at the segment
// joints, 13 doubles each), which tests/test_cloud_prior_shim.py compares with the Python path; exit code 3 when the device
// is missing.
#include <mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h>

#include <cstdlib>
#include <fstream>

int main(int argc, char **argv) {
  if (argc < 26) { printf("usage\n"); return 2; }
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
  const bool use_3d = atoi(argv[25]) != 0;

  std::unique_ptr<MPL::EllipsoidPlanner> planner_;
  planner_.reset(new MPL::EllipsoidPlanner(true));
  planner_->setMap(map, robot_radius, origin, dim);  // Set collision checking function
  planner_->setEpsilon(epsilon);                     // Set greedy param (default equal to 1)
  planner_->setVmax(v_max);                          // Set max velocity
  planner_->setAmax(a_max);                          // Set max acceleration
  planner_->setDt(dt);                               // Set dt for each primitive
  planner_->setW(w);                                 // Set time weight for each primitive
  planner_->setMaxNum(max_num);                      // Set maximum allowed expansion, -1 means no limitation
  planner_->setTol(2.0, 2.0, 100.0);                 // Tolerance for goal region as pos, vel, acc

  // Set input control
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

  // the prior: the same query in ACC states
  Waypoint3D start;
  start.pos = Vec3f(start_x, start_y, start_z);
  start.vel = Vec3f(0, 0, 0);
  start.acc = Vec3f(0, 0, 0);
  start.jrk = Vec3f(0, 0, 0);
  start.use_pos = true;
  start.use_vel = true;
  start.use_acc = false;
  start.use_jrk = false;
  start.use_yaw = false;
  Waypoint3D goal(start.control);
  goal.pos = Vec3f(goal_x, goal_y, goal_z);
  goal.vel = Vec3f(0, 0, 0);
  goal.acc = Vec3f(0, 0, 0);
  goal.jrk = Vec3f(0, 0, 0);
  const bool valid_prior = planner_->plan(start, goal);
  const mplx_result r0 = planner_->getResult();
  if (!valid_prior && r0.n_expanded == 0 && r0.status == 0) {  // (nothing ran: the device or the map is missing)
    printf("{\"error\": \"not planned\"}\n");
    return 3;
  }
  const Trajectory<3> prior_traj = planner_->getTraj();
  const double prior_cost = planner_->getTrajCost();
  if (!valid_prior || prior_traj.segs.empty()) {
    printf("{\"error\": \"no prior trajectory\"}\n");
    return 4;
  }

  // the guided plan (ellipsoid_planner_node.cpp:95-110,134-138,163)
  start.use_acc = true;
  goal = Waypoint3D(start.control);
  goal.pos = Vec3f(goal_x, goal_y, goal_z);
  goal.vel = Vec3f(0, 0, 0);
  goal.acc = Vec3f(0, 0, 0);
  goal.jrk = Vec3f(0, 0, 0);
  planner_->setPriorTrajectory(prior_traj);
  goal.use_acc = false;
  goal.use_jrk = false;
  const bool valid = planner_->plan(start, goal);
  const mplx_result &r = planner_->getResult();
  const auto traj = planner_->getTraj();
  const double cost = planner_->getTrajCost();
  char cost_s[64];  // (JSON has no inf: Infinity, as Python's json writes and reads it)
  if (std::isinf(cost)) snprintf(cost_s, sizeof(cost_s), "Infinity"); else snprintf(cost_s, sizeof(cost_s), "%.17g", cost);
  printf("{\"prior_cost\": %.17g, \"prior_n_expanded\": %llu, \"prior_traj_len\": %zu, \"valid\": %s, \"status\": %d, \"cost\": %s, "
         "\"n_expanded\": %llu, \"traj_len\": %zu, \"traj\": [",
         prior_cost, (unsigned long long)r0.n_expanded, prior_traj.segs.size(), valid ? "true" : "false", r.status, cost_s,
         (unsigned long long)r.n_expanded, traj.segs.size());
  const auto ws = traj.getWaypoints();
  for (size_t i = 0; i < ws.size(); i++) {
    printf("%s[", i ? ", " : "");
    for (int k = 0; k < 3; k++) printf("%.17g, ", ws[i].pos(k));
    for (int k = 0; k < 3; k++) printf("%.17g, ", ws[i].vel(k));
    for (int k = 0; k < 3; k++) printf("%.17g, ", ws[i].acc(k));
    for (int k = 0; k < 3; k++) printf("%.17g, ", ws[i].jrk(k));
    printf("%.17g]", ws[i].t);
  }
  printf("]}\n");
  return 0;
}
