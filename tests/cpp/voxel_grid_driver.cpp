// One fixed operation sequence through the shim's VoxelGrid (include/mpl_shim/planning_ros_utils/voxel_grid.h): constructor,
// both addCloud forms, decay, fill / clear, allocate, getCloud / getMap / getInflatedMap.  The state after every step is
// printed as one JSON line; tests/test_grid_geometry.py runs the same steps on the oracle and compares.
//
//   voxel_grid_driver ox oy oz sx sy sz res  ax ay az bx by bz  cloud.bin n1 n2
// (origin, metric size, resolution; size and origin of the allocate step; two clouds of n1 and n2 points, f64 x y z)
#include <planning_ros_utils/voxel_grid.h>

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

static void dump_map(const char *key, const planning_ros_msgs::VoxelMap &m) {
  printf("\"%s\": {\"dim\": [%d, %d, %d], \"origin\": [%.17g, %.17g, %.17g], \"res\": %.9g, \"data\": \"", key, (int)m.dim.x, (int)m.dim.y, (int)m.dim.z,
         (double)m.origin.x, (double)m.origin.y, (double)m.origin.z, (double)m.resolution);
  for (signed char v : m.data) printf("%02x", (unsigned)(unsigned char)v);
  printf("\"}");
}
static void dump(const char *step, VoxelGrid &g, const vec_Vec3i *new_obs, int flag) {
  printf("{\"step\": \"%s\", \"flag\": %d, \"new_obs\": [", step, flag);
  if (new_obs)
    for (size_t i = 0; i < new_obs->size(); i++) printf("%s[%d, %d, %d]", i ? ", " : "", (*new_obs)[i](0), (*new_obs)[i](1), (*new_obs)[i](2));
  printf("], ");
  dump_map("map", g.getMap());
  printf(", ");
  dump_map("inflated", g.getInflatedMap());
  printf(", \"cloud\": [");
  vec_Vec3f c = g.getCloud();
  for (size_t i = 0; i < c.size(); i++) printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", c[i](0), c[i](1), c[i](2));
  printf("]}\n");
}

int main(int argc, char **argv) {
  if (argc != 17) {
    fprintf(stderr, "usage: %s ox oy oz sx sy sz res ax ay az bx by bz cloud.bin n1 n2\n", argv[0]);
    return 2;
  }
  double a[13];
  for (int i = 0; i < 13; i++) a[i] = strtod(argv[1 + i], nullptr);
  const int n1 = atoi(argv[15]), n2 = atoi(argv[16]);
  std::vector<double> raw(3 * (size_t)(n1 + n2));
  FILE *f = fopen(argv[14], "rb");
  if (!f || fread(raw.data(), sizeof(double), raw.size(), f) != raw.size()) {
    fprintf(stderr, "cannot read %s\n", argv[14]);
    return 2;
  }
  fclose(f);
  vec_Vec3f pts1, pts2;
  for (int i = 0; i < n1 + n2; i++) (i < n1 ? pts1 : pts2).push_back(Vec3f(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]));
  vec_Vec3i ns18, ring;
  for (int x = -1; x <= 1; x++)
    for (int y = -1; y <= 1; y++)
      for (int z = 0; z <= 1; z++) ns18.push_back(Vec3i(x, y, z));
  for (int x = -3; x <= 3; x += 3)
    for (int y = -3; y <= 3; y += 3)
      for (int z = -3; z <= 3; z += 3)
        if (x || y || z) ring.push_back(Vec3i(x, y, z));
  try {
    VoxelGrid g(Vec3f(a[0], a[1], a[2]), Vec3f(a[3], a[4], a[5]), (float)a[6]);
    dump("constructor", g, nullptr, 0);
    g.addCloud(pts1);
    dump("addCloud", g, nullptr, 0);
    vec_Vec3i obs = g.addCloud(pts2, ns18);
    dump("addCloud_ns", g, &obs, 0);
    g.decay();
    dump("decay", g, nullptr, 0);
    g.fill(2, 1);
    g.fill(0, 0, 0);
    g.fill(-1, 0);
    g.fill(1, 1, 400);
    g.clear(3, 2);
    dump("fill_clear", g, nullptr, 0);
    obs = g.addCloud(pts2, ns18);  // the cells that decayed to 99 flip again
    dump("addCloud_ns_again", g, &obs, 0);
    bool ch = g.allocate(Vec3f(a[7], a[8], a[9]), Vec3f(a[10], a[11], a[12]));
    dump("allocate", g, nullptr, ch ? 1 : 0);
    ch = g.allocate(Vec3f(a[7], a[8], a[9]), Vec3f(a[10], a[11], a[12]));
    dump("allocate_same", g, nullptr, ch ? 1 : 0);
    obs = g.addCloud(pts1, ring);
    dump("addCloud_ring", g, &obs, 0);
    g.clear();
    dump("clear", g, nullptr, 0);
  } catch (const std::exception &e) {
    printf("error: %s\n", e.what());  // plain text, not a JSON line: the message is not escaped
    return 3;
  }
  return 0;
}
