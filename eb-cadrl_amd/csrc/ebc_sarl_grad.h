// ebc_sarl_grad.h — the SARL value network's forward over every row of a chunk's states and the backward through all of
// it, as ONE kernel, and the small kernel that adds the chunks' partials: the arithmetic of ebc_sarl_grad_rule.h, byte for
// byte.
//
// A workgroup of eight waves owns one chunk of EBC_SARL_GRAD_CHUNK consecutive states; a state's R row slots lie side by
// side (slot q = state * R + row; the slots at or past a state's n hold zeros in X and enter no sum).
//   layer     grad_layer (ebc_grad_common.h, as grad_dw and grad_dx): a thread owns (a tile of 4 slots, unit u); the weights
//             W[k][u] come from the packed image in global memory (L2; adjacent lanes read adjacent floats), the inputs are LDS broadcasts.  Attention's layer 0
//             reads its second half (the mean) per state.
//   glue      the mean, the softmax (a thread per state, rows ascending), the weighted sum: the rule's chains as written.
//   dW, db    grad_dw: a thread owns entries (k, u) of a layer; its chain runs over the chunk's live states ascending and
//             a state's rows ascending from 0 and is stored ONCE into the chunk's partial.
//   dx        grad_dx: a thread owns (slot, input k); the chain over the layer's units runs ascending from 0.  The result
//             OVERWRITES the ReLU output it is masked by: that activation was the input of this layer's dW, which has
//             finished (a barrier lies between), and nothing else reads it.
// The partials [chunks][packed floats] are then added by grad_reduce (ebc_grad_common.h): one thread per weight, chunks
// ascending, in float64, rounded once.  No atomics, no polling: which workgroup runs a chunk, and when, cannot reach a sum.
//
// LDS, in floats (sarl_grad_lds_floats): per slot X [T padded], A1, H1, B1, FT, C1, C2 [units padded], the score (later its
// delta) and the weight; per state the mean G (later the mean's delta), the joint vector J, its delta DWF, M1, M2, M3,
// the output, the seed, the loss and two ints.  At the reference widths 622 floats per slot and 566 per state: 59 KB at
// R = 5, 109 KB at R = 10, and R <= 15 (158 KB) fits the 160 KB of a gfx950 workgroup.  The weights (381 KB at the reference widths) stay in L2.
//
// Passes (sarl_grad_kernel<true>): the chunk's states run SP in {4, 2, 1} at a time, LDS sized for SP states, so that more
// rows fit (R <= 32 at SP = 2, 64 at SP = 1 at the reference widths).  A pass is the whole forward and backward of its
// states; the thread that owns entries (k, u) of a layer owns them in every pass, and from the second pass on it loads
// its entries from the chunk's partial (global memory, its own earlier store) and continues the fmaf chain where the
// pass before left it: the same chain, the same bytes, whatever SP.  The chunk's float64 loss and count carry on in the
// same way with thread 0.  The first pass always has a state and starts every chain at 0, live or not.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_grad_common.h"
#include "ebc_sarl_grad_rule.h"

#define EBC_SARL_GRAD_WAVES 8
#define EBC_SARL_GRAD_LDS_BYTES (160 * 1024)

namespace ebc {

struct SarlGradLaunch {
  const float *rows;          // [B][R][T]
  const long long *n_valid;   // [B] or nullptr = R
  const float *target;        // [B]
  const unsigned char *mask;  // [B] or nullptr
  float *value;               // [B] or nullptr
  float *attention;           // [B][R] or nullptr
  float *partial;             // [chunks of this launch][D.floats]
  double *loss_part;          // [chunks of this launch]
  long long *count_part;      // [chunks of this launch]
  float grad_scale;
  int B, R;
  int chunk0;                 // the first chunk of this launch
  int SP;                     // states per pass: 4, 2 or 1 (read by the pass form only)
  ebc_sarl::GradDims D;
};

struct SarlGradLds {
  float *X, *A1, *H1, *B1, *FT, *C1, *C2, *SC, *WT, *G, *J, *DWF, *M1, *M2, *M3, *OUT, *SEED;
  double *LOSS;
  int *LIVE, *N;
  int Tp, Jp;
};
// the floats of LDS for SP states at a time (SP = the chunk: the whole chunk at once); the arrays that are SP * R or SP long
// are padded to 4 floats each, so that what follows them keeps its 16-byte (LOSS: 8-byte) alignment at every SP and R
__host__ __device__ inline size_t sarl_grad_lds_floats(const ebc_sarl::GradDims &D, int R, int SP = EBC_SARL_GRAD_CHUNK) {
  using namespace ebc_sarl;
  const size_t slot = (size_t)pad4(D.T) + D.Op[L_M1A] + D.Op[L_M1B] + D.Op[L_M2A] + D.Op[L_M2B] + D.Op[L_ATA] + D.Op[L_ATB];
  const size_t state = (size_t)D.Op[L_M1B] + pad4(D.K[L_M3A]) + D.Op[L_M2B] + D.Op[L_M3A] + D.Op[L_M3B] + D.Op[L_M3C];
  return (size_t)SP * R * slot + 2 * (size_t)pad4(SP * R) + SP * state + 4 * (size_t)pad4(SP) + pad4(2 * SP);
}
// the largest R at which SP states fit a workgroup's LDS (0: not even one row)
__host__ __device__ inline int sarl_grad_max_rows(const ebc_sarl::GradDims &D, int SP = EBC_SARL_GRAD_CHUNK) {
  int R = 0;
  while (R < 1024 && sarl_grad_lds_floats(D, R + 1, SP) * sizeof(float) <= EBC_SARL_GRAD_LDS_BYTES) ++R;
  return R;
}
__device__ __forceinline__ SarlGradLds sarl_grad_lds(float *p, const ebc_sarl::GradDims &D, int R, int SP) {
  using namespace ebc_sarl;
  const int NR = SP * R, NRp = pad4(NR), SPp = pad4(SP);
  SarlGradLds L;
  L.Tp = pad4(D.T), L.Jp = pad4(D.K[L_M3A]);
  L.X = p, p += NR * L.Tp;
  L.A1 = p, p += NR * D.Op[L_M1A];
  L.H1 = p, p += NR * D.Op[L_M1B];
  L.B1 = p, p += NR * D.Op[L_M2A];
  L.FT = p, p += NR * D.Op[L_M2B];
  L.C1 = p, p += NR * D.Op[L_ATA];
  L.C2 = p, p += NR * D.Op[L_ATB];
  L.SC = p, p += NRp;
  L.WT = p, p += NRp;
  L.G = p, p += SP * D.Op[L_M1B];
  L.J = p, p += SP * L.Jp;
  L.DWF = p, p += SP * D.Op[L_M2B];
  L.M1 = p, p += SP * D.Op[L_M3A];
  L.M2 = p, p += SP * D.Op[L_M3B];
  L.M3 = p, p += SP * D.Op[L_M3C];
  L.OUT = p, p += SPp;
  L.SEED = p, p += SPp;
  L.LOSS = reinterpret_cast<double *>(p), p += pad4(2 * SP);  // every array is a multiple of 4 floats long: so is every offset
  L.LIVE = reinterpret_cast<int *>(p), p += SPp;
  L.N = reinterpret_cast<int *>(p);
  return L;
}

constexpr int kSarlNT = 64 * EBC_SARL_GRAD_WAVES;

// instantiated here, ahead of the two kernels, so that the unit's code object lays its kernels out as it did when the
// reduction was this header's own: behind them it cost the default call 0.3 % at B = 4096 (profiles/grad_refactor.txt)
template __global__ void grad_reduce<true>(const float *__restrict__, const double *__restrict__, const long long *__restrict__, int, size_t, int, int,
                                           double *, float *, double *, long long *);

// PASSES false: the whole chunk at once.  true: a.SP states at a time (see "Passes" above).
template <bool PASSES>
__global__ __launch_bounds__(kSarlNT) void sarl_grad_kernel(const float *__restrict__ P, const SarlGradLaunch a) {
  extern __shared__ float4 sarl_grad_lds4[];
  constexpr int C = EBC_SARL_GRAD_CHUNK, NT = kSarlNT;
  using namespace ebc_sarl;
  const GradDims &D = a.D;
  const int tid = threadIdx.x, R = a.R, T = D.T, S = D.S;
  const int SP = PASSES ? a.SP : C;
  const SarlGradLds L = sarl_grad_lds(reinterpret_cast<float *>(sarl_grad_lds4), D, R, SP);
  const int Tp = L.Tp, Jp = L.Jp;
  const int O0 = D.Op[L_M1A], O1 = D.Op[L_M1B], O2 = D.Op[L_M2A], O3 = D.Op[L_M2B], O4 = D.Op[L_ATA], O5 = D.Op[L_ATB];
  const int O7 = D.Op[L_M3A], O8 = D.Op[L_M3B], O9 = D.Op[L_M3C];
  const int H = D.O[L_M1B], F = D.O[L_M2B], KG = D.global ? H : 0;
  const long long chunk_at = ((long long)a.chunk0 + blockIdx.x) * C;
  const int chunk_n = a.B - chunk_at < C ? (int)(a.B - chunk_at) : C;  // states of this chunk, >= 1
  float *const part = a.partial + (size_t)blockIdx.x * D.floats;
#define AT(l) (P + D.at[l])
#define GAT(l) (part + D.at[l])

  int at = 0;  // the pass's first state in the chunk
  do {
    const bool cont = PASSES && at > 0;
    const long long c0 = chunk_at + at;
    const int nc = chunk_n - at < SP ? chunk_n - at : SP;  // states of this pass, >= 1
    const int nq = nc * R;

    // ---- the states' row counts; the rows (zeros in the slots a state does not have: those are never read from memory)
    grad_load_rows<NT>(a, L, c0, nc, SP, T);
    __syncthreads();

    // ---- forward: mlp1, mlp2
    grad_layer<NT, true>(AT(L_M1A), T, 0, D.O[L_M1A], O0, L.X, Tp, nullptr, 0, R, L.A1, O0, nq);
    __syncthreads();
    grad_layer<NT, true>(AT(L_M1B), D.K[L_M1B], 0, H, O1, L.A1, O0, nullptr, 0, R, L.H1, O1, nq);
    __syncthreads();
    grad_layer<NT, true>(AT(L_M2A), H, 0, D.O[L_M2A], O2, L.H1, O1, nullptr, 0, R, L.B1, O2, nq);
    if (D.global)
      for (int i = tid; i < nc * H; i += NT) {
        const int s = i / H, k = i - s * H, n = L.N[s];
        if (n < 1) continue;
        float acc = 0.0f;
        for (int r = 0; r < n; ++r) acc = acc + L.H1[(s * R + r) * O1 + k];
        L.G[s * O1 + k] = over_rows(acc, n);
      }
    __syncthreads();
    grad_layer<NT, false>(AT(L_M2B), D.K[L_M2B], 0, F, O3, L.B1, O2, nullptr, 0, R, L.FT, O3, nq);
    // ---- attention
    grad_layer<NT, true>(AT(L_ATA), H, KG, D.O[L_ATA], O4, L.H1, O1, L.G, O1, R, L.C1, O4, nq);
    __syncthreads();
    grad_layer<NT, true>(AT(L_ATB), D.K[L_ATB], 0, D.O[L_ATB], O5, L.C1, O4, nullptr, 0, R, L.C2, O5, nq);
    __syncthreads();
    grad_layer<NT, false>(AT(L_ATC), D.K[L_ATC], 0, 1, D.Op[L_ATC], L.C2, O5, nullptr, 0, R, L.SC, 1, nq);
    __syncthreads();
    if (tid < nc) {
      const int n = L.N[tid], q0 = tid * R;
      float sum = 0.0f;
      for (int r = 0; r < n; ++r) {
        const float e = score_exp(L.SC[q0 + r]);
        L.WT[q0 + r] = e;
        sum = sum + e;
      }
      for (int r = 0; r < n; ++r) L.WT[q0 + r] = quotient(L.WT[q0 + r], sum);
      if (a.attention)
        for (int r = 0; r < R; ++r) a.attention[(size_t)(c0 + tid) * R + r] = r < n ? canon(L.WT[q0 + r]) : 0.0f;
    }
    __syncthreads();
    // ---- the joint vector: the self state of row 0 and the weighted feature
    for (int i = tid; i < nc * (S + F); i += NT) {
      const int s = i / (S + F), k = i - s * (S + F);
      float v;
      if (k < S) {
        v = L.X[(s * R) * Tp + k];
      } else {
        v = 0.0f;
        for (int r = 0; r < L.N[s]; ++r) v = chain(L.WT[s * R + r], L.FT[(s * R + r) * O3 + (k - S)], v);
      }
      L.J[s * Jp + k] = v;
    }
    __syncthreads();
    // ---- mlp3
    grad_layer<NT, true>(AT(L_M3A), S + F, 0, D.O[L_M3A], O7, L.J, Jp, nullptr, 0, 1, L.M1, O7, nc);
    __syncthreads();
    grad_layer<NT, true>(AT(L_M3B), D.K[L_M3B], 0, D.O[L_M3B], O8, L.M1, O7, nullptr, 0, 1, L.M2, O8, nc);
    __syncthreads();
    grad_layer<NT, true>(AT(L_M3C), D.K[L_M3C], 0, D.O[L_M3C], O9, L.M2, O8, nullptr, 0, 1, L.M3, O9, nc);
    __syncthreads();
    grad_layer<NT, false>(AT(L_M3D), D.K[L_M3D], 0, 1, D.Op[L_M3D], L.M3, O9, nullptr, 0, 1, L.OUT, 1, nc);
    __syncthreads();

    // ---- the values and the seeds, a thread per state; the chunk's loss in state order: thread 0's
    grad_seed(a, L, c0, nc, SP, cont);

    // ---- backward: mlp3
    grad_dw<NT>(GAT(L_M3D), D.K[L_M3D], 0, 1, D.Op[L_M3D], L.SEED, 1, L.M3, O9, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_M3D), 0, D.K[L_M3D], 1, D.Op[L_M3D], L.SEED, 1, L.M3, O9, R, nc, L.N, L.LIVE, false, false);
    __syncthreads();
    grad_dw<NT>(GAT(L_M3C), D.K[L_M3C], 0, D.O[L_M3C], O9, L.M3, O9, L.M2, O8, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_M3C), 0, D.K[L_M3C], D.O[L_M3C], O9, L.M3, O9, L.M2, O8, R, nc, L.N, L.LIVE, false, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_M3B), D.K[L_M3B], 0, D.O[L_M3B], O8, L.M2, O8, L.M1, O7, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_M3B), 0, D.K[L_M3B], D.O[L_M3B], O8, L.M2, O8, L.M1, O7, R, nc, L.N, L.LIVE, false, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_M3A), S + F, 0, D.O[L_M3A], O7, L.M1, O7, L.J, Jp, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, false>(AT(L_M3A), S, S + F, D.O[L_M3A], O7, L.M1, O7, L.DWF, O3, R, nc, L.N, L.LIVE, false, true);  // dwf; J keeps wf
    __syncthreads();

    // ---- the weighted sum and the softmax
    for (int q = tid; q < nq; q += NT) {
      const int s = q / R;
      if (!L.LIVE[s] || q - s * R >= L.N[s]) continue;
      float acc = 0.0f;
      for (int f = 0; f < F; ++f) acc = chain(L.DWF[s * O3 + f], centred(L.FT[q * O3 + f], L.J[s * Jp + S + f]), acc);
      L.SC[q] = acc;
    }
    __syncthreads();
    if (tid < nc && L.LIVE[tid]) {
      const int n = L.N[tid], q0 = tid * R;
      float m = 0.0f;
      for (int r = 0; r < n; ++r) m = chain(L.WT[q0 + r], L.SC[q0 + r], m);
      for (int r = 0; r < n; ++r) L.SC[q0 + r] = score_back(L.WT[q0 + r], L.SC[q0 + r], m);
    }
    for (int i = tid; i < nq * F; i += NT) {
      const int q = i / F, f = i - q * F, s = q / R;
      if (!L.LIVE[s] || q - s * R >= L.N[s]) continue;
      L.FT[q * O3 + f] = L.WT[q] * L.DWF[s * O3 + f];
    }
    __syncthreads();

    // ---- mlp2's last layer and attention's last layer
    grad_dw<NT>(GAT(L_M2B), D.K[L_M2B], 0, F, O3, L.FT, O3, L.B1, O2, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    grad_dw<NT>(GAT(L_ATC), D.K[L_ATC], 0, 1, D.Op[L_ATC], L.SC, 1, L.C2, O5, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_M2B), 0, D.K[L_M2B], F, O3, L.FT, O3, L.B1, O2, R, nc, L.N, L.LIVE, true, true);
    grad_dx<NT, true>(AT(L_ATC), 0, D.K[L_ATC], 1, D.Op[L_ATC], L.SC, 1, L.C2, O5, R, nc, L.N, L.LIVE, true, false);
    __syncthreads();
    grad_dw<NT>(GAT(L_M2A), H, 0, D.O[L_M2A], O2, L.B1, O2, L.H1, O1, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    grad_dw<NT>(GAT(L_ATB), D.K[L_ATB], 0, D.O[L_ATB], O5, L.C2, O5, L.C1, O4, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_ATB), 0, D.K[L_ATB], D.O[L_ATB], O5, L.C2, O5, L.C1, O4, R, nc, L.N, L.LIVE, true, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_ATA), H, KG, D.O[L_ATA], O4, L.C1, O4, L.H1, O1, L.G, O1, R, nc, L.N, L.LIVE, true, cont);
    __syncthreads();

    // ---- h1: the mean's delta (into G), then mlp2's layer 0 + attention's layer 0 + the mean
    if (D.global) {
      for (int i = tid; i < nc * H; i += NT) {
        const int k = i / nc, s = i - k * nc, n = L.N[s];
        if (!L.LIVE[s]) continue;
        float dg = 0.0f;
        for (int r = 0; r < n; ++r) dg = dg + grad_dot(AT(L_ATA) + (size_t)(H + k) * O4, L.C1 + (size_t)(s * R + r) * O4, D.O[L_ATA], true);
        L.G[s * O1 + k] = over_rows(dg, n);
      }
      __syncthreads();
    }
    for (int i = tid; i < nq * H; i += NT) {
      const int k = i / nq, q = i - k * nq, s = q / R;
      if (!L.LIVE[s] || q - s * R >= L.N[s]) continue;
      const float d2 = grad_dot(AT(L_M2A) + (size_t)k * O2, L.B1 + (size_t)q * O2, D.O[L_M2A], true);
      const float d4 = grad_dot(AT(L_ATA) + (size_t)k * O4, L.C1 + (size_t)q * O4, D.O[L_ATA], true);
      float *o = L.H1 + (size_t)q * O1 + k;
      *o = h1_back(*o, d2, d4, D.global ? L.G[s * O1 + k] : 0.0f, D.global);
    }
    __syncthreads();

    // ---- mlp1
    grad_dw<NT>(GAT(L_M1B), D.K[L_M1B], 0, H, O1, L.H1, O1, L.A1, O0, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_M1B), 0, D.K[L_M1B], H, O1, L.H1, O1, L.A1, O0, R, nc, L.N, L.LIVE, true, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_M1A), T, 0, D.O[L_M1A], O0, L.A1, O0, L.X, Tp, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    if (PASSES) __syncthreads();  // the next pass's forward overwrites what this dW reads
  } while (PASSES && (at += SP) < chunk_n);
#undef AT
#undef GAT
}

}  // namespace ebc
