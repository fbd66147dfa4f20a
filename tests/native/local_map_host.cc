// Host build of the product's angular local map (eb-cadrl_amd/csrc/ebc_local_map.h) for the CPU tests: the same
// source the device kernel compiles, run pose by pose, so tests/test_local_map_cpu.py can hold it against
// ebcsim/local_map.py and the reference's own outputs (tests/golden/local_map*.npz) without a GPU.
#include <vector>
#include "../../eb-cadrl_amd/csrc/ebc_local_map.h"

// pose [n][4] = px, py, radius, theta; poly [n_poly][4][2] shared by the n poses; out [n][dim]
extern "C" void local_map_host(const double *poly, int n_poly, const double *pose, int n, int dim, double max_range,
                               double angle_min, double angle_max, int normalize, double *out) {
  const ebc::LocalMapCfg c = ebc::local_map_cfg(dim, max_range, angle_min, angle_max, normalize);
  for (int r = 0; r < n; ++r) {
    const double *q = pose + (size_t)r * 4;
    ebc::local_map_env(c, poly, n_poly, q[0], q[1], q[2], q[3], out + (size_t)r * dim);
  }
}

extern "C" void sincos_dd_host(double angle, double *c, double *s) { ebc::sincos_dd(angle, *c, *s); }

// The generator's polygons of n scenes (ebc_scene_gen.h): poly [n][S][4][2], n_poly [n]; the other outputs are dropped.
extern "C" int scene_gen_poly_host(const EbcSceneGen *gen, const uint32_t *seeds, int n, int N, int S, int G,
                                   double *poly, int *n_poly) {
  std::vector<uint32_t> mt(624);
  const int S1 = S ? S : 1;
  std::vector<double> h((size_t)N * 8), st((size_t)S1 * 3), robot(9);
  std::vector<uint8_t> type(N);
  std::vector<uint64_t> grid((size_t)G * 2);
  int status = 0, nh = 0, ns = 0;
  for (int r = 0; r < n; ++r) {
    ebc::SceneRow o = {&nh, &h[0], &h[N], &h[2 * N], &h[3 * N], &h[4 * N], &h[5 * N], &h[6 * N], &h[7 * N], type.data(),
                       &ns, &st[0], &st[S1], &st[2 * S1], grid.data(), robot.data(),
                       poly + (size_t)r * S1 * 8, n_poly + r};
    status |= ebc::generate_scene_row(*gen, seeds[r], mt.data(), 1, o, N, S, G);
  }
  return status;
}
