// Host build of the product's occupancy-map rule (eb-cadrl_amd/csrc/ebc_om_rule.h) for the tests: the same source the
// kernel compiles, applied serially per env, so tests/test_om_cpu.py can hold it against ebcsim.occupancy.occupancy_maps
// without a GPU and tests/test_om_gpu.py can hold the kernel against it byte for byte.
//
// Built as a shared library (om_host below) and as a program of its own:
//   om_host IN OUT    IN:  int32 count, then per batch int32 E, A, R, T, cell_num, channels, has_n_valid, has_rows;
//                          float64 cell_size; float64 next_ob[E*R*5]; int64 n_valid[E] when has_n_valid;
//                          float32 rows[E*A*R*T] when has_rows
//                     OUT: per batch float32 om[E*R*W]; float32 rows_wide[E*A*R*(T+W)] when has_rows
// which is what the sanitizer build runs (g++ -fsanitize=address,undefined).
#include <stdio.h>

#include <vector>

#include "../../eb-cadrl_amd/csrc/ebc_om_rule.h"

// next_ob [E][R][5]; n_valid [E] int64 or NULL = R; rows [E][A][R][T] or NULL -> om [E][R][W] (or NULL), rows_wide
// [E][A][R][T + W] (or NULL); W = cell_num^2 * channels
extern "C" void om_host(const double *next_ob, const long long *n_valid, const float *rows, int E, int A, int R, int T,
                        int cell_num, double cell_size, int channels, float *om, float *rows_wide) {
  const int cells = cell_num * cell_num, W = cells * channels;
  std::vector<float> maps((size_t)R * W);
  for (int e = 0; e < E; ++e) {
    const double *ob = next_ob + (size_t)e * R * 5;
    const int n = ebc_om::clamp_rows(n_valid ? n_valid[e] : (long long)R, R);
    for (int r = 0; r < R; ++r) {
      float *row = maps.data() + (size_t)r * W;
      if (r >= n) {
        for (int i = 0; i < W; ++i) row[i] = 0.0f;
        continue;
      }
      const ebc_om::Frame f = ebc_om::frame(ob[(size_t)r * 5 + 2], ob[(size_t)r * 5 + 3]);
      for (int k = 0; k < cells; ++k)
        ebc_om::finished_cell(ob, ob + 1, ob + 2, ob + 3, 5, n, r, f, k, cell_num, cell_size, channels, row + (size_t)k * channels);
    }
    if (om) memcpy(om + (size_t)e * R * W, maps.data(), maps.size() * sizeof(float));
    if (rows_wide && rows) {
      for (size_t q = 0; q < (size_t)A * R; ++q) {
        float *dst = rows_wide + ((size_t)e * A * R + q) * (T + W);
        memcpy(dst, rows + ((size_t)e * A * R + q) * T, (size_t)T * sizeof(float));
        memcpy(dst + T, maps.data() + (q % R) * W, (size_t)W * sizeof(float));
      }
    }
  }
}

namespace {

template <typename V>
bool read_n(FILE *f, std::vector<V> &out, size_t n) {
  out.resize(n);
  return n == 0 || fread(out.data(), sizeof(V), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb"), *out = in ? fopen(argv[2], "wb") : nullptr;
  if (!in || !out) {
    fprintf(stderr, "cannot open %s\n", in ? argv[2] : argv[1]);
    if (in) fclose(in);
    return 2;
  }
  int rc = 0, count = 0;
  if (fread(&count, sizeof(int), 1, in) != 1) rc = 1;
  for (int b = 0; !rc && b < count; ++b) {
    int head[8];
    double cell_size;
    if (fread(head, sizeof(int), 8, in) != 8 || fread(&cell_size, sizeof(double), 1, in) != 1) {
      rc = 1;
      break;
    }
    const int E = head[0], A = head[1], R = head[2], T = head[3], cell_num = head[4], channels = head[5];
    if (E < 0 || R < 1 || R > EBC_OM_MAX_ROWS || cell_num < 1 || channels < 1 || channels > 3 ||
        (long long)cell_num * cell_num * channels > EBC_OM_MAX_WIDTH || !(cell_size > 0.0) ||
        (head[7] && (A < 1 || A > EBC_OM_MAX_ACTIONS || T < 1 || T + cell_num * cell_num * channels > EBC_OM_MAX_ROW_WIDTH))) {
      rc = 1;
      break;
    }
    const size_t W = (size_t)cell_num * cell_num * channels, rows_n = head[7] ? (size_t)E * A * R * T : 0;
    std::vector<double> next_ob;
    std::vector<long long> n_valid;
    std::vector<float> rows;
    if (!read_n(in, next_ob, (size_t)E * R * 5) || (head[6] && !read_n(in, n_valid, (size_t)E)) || !read_n(in, rows, rows_n)) {
      rc = 1;
      break;
    }
    std::vector<float> om((size_t)E * R * W), wide(head[7] ? (size_t)E * A * R * (T + W) : 0);
    om_host(next_ob.data(), head[6] ? n_valid.data() : nullptr, head[7] ? rows.data() : nullptr, E, A, R, T, cell_num, cell_size,
            channels, om.data(), head[7] ? wide.data() : nullptr);
    if (fwrite(om.data(), sizeof(float), om.size(), out) != om.size() ||
        (wide.size() && fwrite(wide.data(), sizeof(float), wide.size(), out) != wide.size()))
      rc = 1;
  }
  fclose(in);
  if (fclose(out) != 0) rc = 1;
  if (rc) fprintf(stderr, "malformed input or short write\n");
  else printf("om_host: %d batches\n", count);
  return rc;
}
