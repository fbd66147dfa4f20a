// ebcsim_om.hip — the occupancy maps of OM-SARL (rl/policy/multi_human_rl.py:62-69, :156-227): ebc_occupancy_rows.  Its
// own translation unit beside the simulation path, the two-layer blocks, the LSTM scan and the CADRL decision.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ebc_host.h"
#include "ebc_om.h"

using ebc_host::fail;

extern "C" int ebc_occupancy_rows(int device_id, void *stream, const EbcOmArgs *args) {
  if (!args || args->struct_size != sizeof(EbcOmArgs)) return fail(EBC_ERR_INVALID, "EbcOmArgs.struct_size");
  const std::string who = "ebc_occupancy_rows: ";
  if (!args->next_ob || args->E < 0 || args->R < 1) return fail(EBC_ERR_INVALID, who + "next_ob, E, R");
  if (!args->om && !args->rows_wide) return fail(EBC_ERR_UNSUPPORTED, who + "no output (om and rows_wide are both NULL)");
  if (args->rows_wide && !args->rows) return fail(EBC_ERR_UNSUPPORTED, who + "rows_wide without rows");
  if (args->channels < 1 || args->channels > 3)
    return fail(EBC_ERR_UNSUPPORTED, who + "channels not in {1, 2, 3} (" + std::to_string(args->channels) + ")");
  if (args->cell_num < 1) return fail(EBC_ERR_UNSUPPORTED, who + "cell_num < 1 (" + std::to_string(args->cell_num) + ")");
  if (!(std::isfinite(args->cell_size) && args->cell_size > 0.0)) return fail(EBC_ERR_UNSUPPORTED, who + "cell_size is not a finite positive number");
  const long long W = (long long)args->cell_num * args->cell_num * args->channels;
  if (W > EBC_OM_MAX_WIDTH) return fail(EBC_ERR_UNSUPPORTED, who + "W > 192 map columns (" + std::to_string(W) + ")");
  if (args->R > EBC_OM_MAX_ROWS) return fail(EBC_ERR_UNSUPPORTED, who + "R > 128 row slots (" + std::to_string(args->R) + ")");
  if (args->rows_wide) {
    if (args->A < 1 || args->T < 1) return fail(EBC_ERR_INVALID, who + "A, T");
    if (args->A > EBC_OM_MAX_ACTIONS) return fail(EBC_ERR_UNSUPPORTED, who + "A > 128 actions (" + std::to_string(args->A) + ")");
    if (args->T + W > EBC_OM_MAX_ROW_WIDTH)
      return fail(EBC_ERR_UNSUPPORTED, who + "T + W > 224 columns, the blocks' input limit (" + std::to_string(args->T + W) + ")");
  }
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
    return fail(EBC_ERR_UNSUPPORTED, who + "the stream is being captured into a HIP graph; the maps must be launched, not replayed");
  if (args->E == 0) return EBC_OK;
  HIP_TRY(hipSetDevice(device_id));
  ebc::OmLaunch a;
  a.next_ob = args->next_ob;
  a.n_valid = reinterpret_cast<const long long *>(args->n_valid);
  a.rows = args->rows;
  a.om = args->om;
  a.rows_wide = args->rows_wide;
  a.cell_size = args->cell_size;
  a.cell_num = args->cell_num;
  a.channels = args->channels;
  a.A = args->rows_wide ? args->A : 0;
  a.R = args->R;
  a.T = args->rows_wide ? args->T : 0;
  const size_t lds = ebc::om_lds_bytes(args->R, (int)W);  // <= 102 KB at R = 128, W = 192
  static size_t raised_dev[64] = {0};  // more than the 64 KB a launch gets by default; a function attribute is per device
  if (lds > 65536 && lds > raised_dev[device_id & 63]) {
    HIP_TRY(hipFuncSetAttribute((const void *)ebc::occupancy_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised_dev[device_id & 63] = lds;
  }
  // The shares of an env's actions: enough workgroups to keep every CU streaming, at most 8 per env (each computes the
  // env's maps again) and one where the maps are the larger part of the work.
  int shares = 1;
  if (args->rows_wide) {
    const long long want = (2048 + args->E - 1) / args->E;
    shares = (int)(want < 1 ? 1 : want > 8 ? 8 : want);
    if (shares > args->A) shares = args->A;
    if ((long long)args->R * args->R * args->cell_num * args->cell_num > (long long)args->A * args->R * (args->T + W)) shares = 1;
  }
  hipLaunchKernelGGL(ebc::occupancy_rows_kernel, dim3((unsigned)args->E, (unsigned)shares), dim3(EBC_OM_THREADS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return EBC_OK;
}
