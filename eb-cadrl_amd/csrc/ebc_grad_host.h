// ebc_grad_host.h — the host side the gradient units share (ebcsim_cadrl_grad.hip, ebcsim_sarl_grad.hip,
// ebcsim_lstm_grad.hip, ebcsim_sail_grad.hip): what a network object owns and its ebc_*_net_* entries' bodies (GradNet),
// the row limits of the kernels that run a chunk's states in passes (GradPasses), and the chunk launcher (grad_launch:
// chunk counts, the scratch's layout, the loop of main kernel and grad_reduce).  `what` is the entry's name, for its texts.
#pragma once

#include <vector>

#include "ebc_grad_common.h"
#include "ebc_host.h"

namespace ebc_host {

// what every network object owns; CadrlNet, SarlNet and LstmNet derive from it and add their GradDims
struct GradNet {
  int device = 0;
  float *P = nullptr;       // the packed image
  size_t floats = 0;        // its length
  void *scratch = nullptr;  // float64 sums | chunk losses | chunk counts | chunk partials
  size_t scratch_bytes = 0;
};

// the image into device memory and the new object out; a failure deletes the object
template <class Net>
int grad_net_upload(Net *n, const std::vector<float> &image, const std::string &what, void **net_out) {
  n->floats = image.size();
  hipError_t err = hipMalloc(&n->P, image.size() * sizeof(float));
  if (err == hipSuccess) err = hipMemcpy(n->P, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (n->P) (void)hipFree(n->P);
    delete n;
    return fail(EBC_ERR_DEVICE, what + ": " + hipGetErrorString(err));
  }
  *net_out = n;
  return EBC_OK;
}

template <class Net>
int grad_net_destroy(Net *n) {
  if (!n) return EBC_OK;
  (void)hipSetDevice(n->device);
  if (n->scratch) (void)hipFree(n->scratch);
  if (n->P) (void)hipFree(n->P);
  delete n;
  return EBC_OK;
}

inline int grad_net_packed_floats(const GradNet *n, int64_t *floats_out, const std::string &what) {
  if (!n || !floats_out) return fail(EBC_ERR_INVALID, what + ": null argument");
  *floats_out = (int64_t)n->floats;
  return EBC_OK;
}

// get_packed (dst_dev) and set_packed (src_dev): the one that is given is the other end of the copy
inline int grad_net_copy_packed(GradNet *n, void *stream, float *dst_dev, const float *src_dev, const std::string &what) {
  if (!n || (!dst_dev && !src_dev)) return fail(EBC_ERR_INVALID, what + ": null argument");
  if (capturing(stream)) return fail(EBC_ERR_UNSUPPORTED, what + ": the stream is being captured into a HIP graph");
  HIP_TRY(hipSetDevice(n->device));
  float *const dst = dst_dev ? dst_dev : n->P;
  const float *const src = src_dev ? src_dev : n->P;
  HIP_TRY(hipMemcpyAsync(dst, src, n->floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EBC_OK;
}

// the network's scratch, at least `need` bytes: grows on demand; growing waits for the device (work that reads the old
// scratch may be in flight)
inline int grad_net_scratch(GradNet *n, size_t need, void **out) {
  if (need > n->scratch_bytes) {
    HIP_TRY(hipDeviceSynchronize());
    if (n->scratch) HIP_TRY(hipFree(n->scratch));
    n->scratch = nullptr;
    n->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&n->scratch, need));
    n->scratch_bytes = need;
  }
  *out = n->scratch;
  return EBC_OK;
}

// the largest R a kernel that runs a chunk's states in passes takes: the whole chunk at once, and 4, 2, 1 states per pass
struct GradPasses {
  int max_rows = 0;                // the largest R whose chunk fits a workgroup's LDS
  int max_rows_at[3] = {0, 0, 0};  // the same with 4, 2, 1 states per pass

  // states_per_pass 4, 2, 1 -> 0, 1, 2; anything else -1
  static int pass_index(int states_per_pass) { return states_per_pass == 4 ? 0 : states_per_pass == 2 ? 1 : states_per_pass == 1 ? 2 : -1; }

  // max_rows_of(states per pass): the kernel's own LDS arithmetic
  template <class F>
  void fill(int chunk, F max_rows_of) {
    max_rows = max_rows_of(chunk);
    for (int sp = 4, i = 0; sp >= 1; sp /= 2, ++i) max_rows_at[i] = max_rows_of(sp);
  }

  // states_per_pass is 0 (the whole chunk at once, the kernel's default call), 4, 2 or 1
  static int check(int states_per_pass, const std::string &what) {
    if (states_per_pass != 0 && pass_index(states_per_pass) < 0)
      return fail(EBC_ERR_INVALID, what + ": states_per_pass " + std::to_string(states_per_pass) + " is none of 0, 4, 2, 1");
    return EBC_OK;
  }

  int limit(int states_per_pass) const { return states_per_pass == 0 ? max_rows : max_rows_at[pass_index(states_per_pass)]; }

  // R rows per state against the limit of a checked states_per_pass; lds_kb: a workgroup's LDS
  int refuse_rows(int R, int states_per_pass, int lds_kb, const std::string &what) const {
    if (R <= limit(states_per_pass)) return EBC_OK;
    if (states_per_pass == 0)
      return fail(EBC_ERR_UNSUPPORTED, what + ": R = " + std::to_string(R) + " row slots per state, a chunk of this network fits a workgroup's " +
                                           std::to_string(lds_kb) + " KB of LDS up to R = " + std::to_string(max_rows));
    return fail(EBC_ERR_UNSUPPORTED, what + ": R = " + std::to_string(R) + " row slots per state with S = " + std::to_string(states_per_pass) +
                                         " states per pass, that many states of this network fit a workgroup's " + std::to_string(lds_kb) +
                                         " KB of LDS up to R = " + std::to_string(limit(states_per_pass)));
  }
};

// the body of ebc_*_net_grad_max_rows_at
inline int grad_max_rows_at(const GradPasses *p, int states_per_pass, int *rows_out, const std::string &what) {
  if (!p || !rows_out) return fail(EBC_ERR_INVALID, what + ": null argument");
  if (int rc = GradPasses::check(states_per_pass, what)) return rc;
  *rows_out = p->limit(states_per_pass);
  return EBC_OK;
}

// One gradient over `units` states (envs) in chunks of `chunk`, at most `max_chunks` chunks of partials per launch before
// the float64 sums take over.  scratch(bytes, &p) hands out the device memory, laid out as float64 sums [PF + 2] |
// loss_part [per] | count_part [per] | partial [per][PF]; main(chunk0, now, partial, loss_part, count_part) launches the
// unit's kernel on `now` chunks from chunk0 on; grad_reduce<CANON> adds their partials into grad, loss_sum and count.
template <bool CANON, class Scratch, class Main>
int grad_launch(hipStream_t st, size_t PF, long long units, int chunk, int max_chunks, Scratch scratch, float *grad, double *loss_sum,
                int64_t *count, Main main) {
  const long long chunks = (units + chunk - 1) / chunk;
  const int per = chunks < max_chunks ? (int)(chunks > 0 ? chunks : 1) : max_chunks;
  const size_t acc_bytes = (PF + 2) * sizeof(double), part_at = acc_bytes + (size_t)per * 16;
  void *mem = nullptr;
  if (int rc = scratch(part_at + (size_t)per * PF * sizeof(float), &mem)) return rc;
  double *acc64 = static_cast<double *>(mem);
  double *loss_part = reinterpret_cast<double *>(static_cast<char *>(mem) + acc_bytes);
  long long *count_part = reinterpret_cast<long long *>(loss_part + per);
  float *partial = reinterpret_cast<float *>(static_cast<char *>(mem) + part_at);
  const unsigned reduce_blocks = (unsigned)((PF + 255) / 256);
  long long done = 0;
  do {
    const int now = chunks - done < per ? (int)(chunks - done) : per;
    if (now > 0) {
      main((int)done, now, partial, loss_part, count_part);
      HIP_TRY(hipGetLastError());
    }
    const int first = done == 0, last = done + now >= chunks;
    hipLaunchKernelGGL(ebc::grad_reduce<CANON>, dim3(reduce_blocks), dim3(256), 0, st, partial, loss_part, count_part, now, PF, first, last, acc64,
                       grad, loss_sum, reinterpret_cast<long long *>(count));
    HIP_TRY(hipGetLastError());
    done += now;
  } while (done < chunks);
  return EBC_OK;
}

}  // namespace ebc_host
