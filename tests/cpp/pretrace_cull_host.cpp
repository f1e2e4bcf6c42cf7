// Host-side check of the fused kernel's pre-trace cull (rpt_amd/csrc/host_scene.cpp pinhole_screen_rect): the Cornell box
// of examples/cornell.rs, built with the C++ mirror's builders and flattened with the PRODUCT's flattener (no GPU); for
// the camera and frame given on the command line (eye, direction, up: 9 numbers, fov, width, height) prints, per object,
// whether the object filter exempts it and the screen rectangle the product computes from its world box.
// Driven by tests/test_pretrace_cull_host.py, which shoots the oracle's camera rays at the oracle's exact tests.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rpt.hpp"
#include "../../rpt_amd/csrc/host_scene.h"

namespace rpthost { // the device builder is not linked into this test: the host builder makes the same tree
bool kd_build_device(const std::vector<Box>&, KdBuild&, int, std::string& why) { why = "not linked"; return false; }
}

int main(int argc, char** argv) {
  using namespace rpt;
  if (argc != 13) return 2;
  const double two_pi = 2.0 * M_PI;
  std::vector<Shape> shapes;
  shapes.push_back(polygon({{0.0, 0.0, 0.0}, {0.0, 0.0, 559.2}, {556.0, 0.0, 559.2}, {556.0, 0.0, 0.0}}));
  shapes.push_back(polygon({{0.0, 548.9, 0.0}, {556.0, 548.9, 0.0}, {556.0, 548.9, 559.2}, {0.0, 548.9, 559.2}}));
  shapes.push_back(polygon({{0.0, 0.0, 559.2}, {0.0, 548.9, 559.2}, {556.0, 548.9, 559.2}, {556.0, 0.0, 559.2}}));
  shapes.push_back(polygon({{556.0, 0.0, 0.0}, {556.0, 0.0, 559.2}, {556.0, 548.9, 559.2}, {556.0, 548.9, 0.0}}));
  shapes.push_back(polygon({{0.0, 0.0, 0.0}, {0.0, 548.9, 0.0}, {0.0, 548.9, 559.2}, {0.0, 0.0, 559.2}}));
  shapes.push_back(cube().scale({165.0, 330.0, 165.0}).rotate_y(two_pi * (-253.0 / 360.0)).translate({368.0, 165.0, 351.0}));
  shapes.push_back(cube().scale({165.0, 165.0, 165.0}).rotate_y(two_pi * (-197.0 / 360.0)).translate({185.0, 82.5, 169.0}));
  Arena arena;
  std::vector<RptObject> objs;
  for (const Shape& s : shapes) objs.push_back({s.lower(arena), Material::diffuse({0.5, 0.5, 0.5}).lower()});
  RptScene sc{};
  sc.objects = objs.data();
  sc.num_objects = objs.size();
  rpthost::FlatScene fs;
  std::string err;
  const int rc = rpthost::flatten_scene(sc, fs, err, nullptr);
  std::printf("rc %d ok %d n %zu always %llx\n", rc, fs.obj_filter_ok ? 1 : 0, fs.obj_geom.size(), (unsigned long long)fs.obj_always);
  rptdev::Camera cam{}; // as api_render.cpp make_camera
  for (int k = 0; k < 3; k++) { cam.eye[k] = std::atof(argv[1 + k]); cam.direction[k] = std::atof(argv[4 + k]); cam.up[k] = std::atof(argv[7 + k]); }
  cam.d = 1.0 / std::tan(std::atof(argv[10]) / 2.0);
  const double* a = cam.direction;
  const double* b = cam.up;
  const double cr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double len = std::sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  for (int k = 0; k < 3; k++) cam.right[k] = cr[k] / len;
  const uint32_t w = (uint32_t)std::atoi(argv[11]), h = (uint32_t)std::atoi(argv[12]);
  for (size_t i = 0; i < fs.obj_geom.size(); i++) {
    uint32_t r[4] = {0, 0, 0, 0};
    const bool got = rpthost::pinhole_screen_rect(rpthost::world_box(fs.obj_geom[i], fs.insts[i]), cam, w, h, r);
    std::printf("rect %zu kind %d got %d x %u %u y %u %u\n", i, (int)fs.insts[i].kind, got ? 1 : 0, r[0], r[1], r[2], r[3]);
  }
  cam.aperture = 1.0; // a lens: no rectangle
  uint32_t r[4];
  std::printf("lens got %d\n", rpthost::pinhole_screen_rect(rpthost::world_box(fs.obj_geom[5], fs.insts[5]), cam, w, h, r) ? 1 : 0);
  return 0;
}
