// ebc_lstm_grad.h — the LSTM-RL value networks' forward over every row of a chunk's states, the recurrence, and the backward
// through all of it (through time included), as ONE kernel, and the small kernel that adds the chunks' partials: the
// arithmetic of ebc_lstm_grad_rule.h, byte for byte.
//
// A workgroup of eight waves owns one chunk of EBC_LSTM_GRAD_CHUNK consecutive states; a state's R row slots lie side by
// side (slot q = state * R + step; the slots at or past a state's n hold zeros in X and enter no sum).
//   layer     grad_layer (ebc_grad_common.h, as grad_dw and grad_dx): a thread owns (a tile of 4 slots, unit u); the weights
//             W[k][u] come from the packed image in global memory (L2; adjacent lanes read adjacent floats), the inputs are LDS broadcasts.
//   step      the recurrence, a step at a time for all states of the chunk that still have one.  Gates: a thread owns (gate
//             row q, a pair of states) and walks the rule's chain over xi[t] and then h[t-1], w_ih[k][q] and w_hh[k][q]
//             read once for the pair (adjacent lanes, adjacent floats).  Cell: a thread owns (state, unit).  What a step
//             keeps (i, f, g, o in the places of their pre-activations, c, tanh(c), h) stays in LDS for the walk back.
//             This is not the forward kernel's sequence-per-lane layout (ebc_lstm.h): a chunk has four sequences.
//   back      per step from the last: a thread owns (state, unit) for the rule's cell_back (the gates become their deltas),
//             then (state, unit k) for dh[k], the chain over all 4 H gate rows of w_hh[k][.] (contiguous in the image).
//   dW, db    grad_dw / the cell's loop: a thread owns entries (k, u) of a layer; its chain runs over the chunk's live states
//             ascending and a state's steps ascending from 0 and is stored ONCE into the chunk's partial.
//   dx        grad_dx: a thread owns (slot, input k); the chain over the layer's units runs ascending from 0.  The result
//             OVERWRITES the ReLU output it is masked by (mlp1's xi: the cell's input it is the gradient of): that activation
//             was the input of this layer's dW, which has finished (a barrier lies between), and nothing else reads it.
// The partials [chunks][packed floats] are then added by grad_reduce (ebc_grad_common.h): one thread per weight, chunks
// ascending, in float64, rounded once.  No atomics, no polling: which workgroup runs a chunk, and when, cannot reach a sum.
//
// LDS, in floats (lstm_grad_lds_floats): per slot X [T padded], with mlp1 A1, A2, A3, XI [units padded], the step's record
// [4 H + 3 H padded]; per state the joint vector J, M1, M2, M3, dh, dc, the output, the seed, the loss and two ints; one
// zero vector (h[-1]).  At the reference widths with mlp1 776 floats per slot and 518 per state: 70 KB at R = 5, 133 KB at
// R = 10, and R <= 12 fits the 160 KB of a gfx950 workgroup; without mlp1 372 per slot and R <= 26.  The weights (349 KB at the
// reference widths) stay in L2.
//
// Passes (lstm_grad_kernel<true>): the chunk's states run SP in {4, 2, 1} at a time, LDS sized for SP states, so that more
// rows fit (R <= 25 at SP = 2, 52 at SP = 1 at the reference widths with mlp1).  A pass is the whole forward, recurrence
// and backward of its states (with SP = 1 the gate step's pair is the one state alone); the thread that owns entries of a
// layer or of the cell's weights owns them in every pass, and from the second pass on it loads them from the chunk's
// partial (global memory, its own earlier store) and continues the fmaf chain where the pass before left it: the same
// chain, the same bytes, whatever SP.  The chunk's float64 loss and count carry on in the same way with thread 0.  The
// first pass always has a state and starts every chain at 0, live or not.
#pragma once

#include <hip/hip_runtime.h>

#include "ebc_grad_common.h"
#include "ebc_lstm_grad_rule.h"

#define EBC_LSTM_GRAD_WAVES 8
#define EBC_LSTM_GRAD_LDS_BYTES (160 * 1024)

namespace ebc {

struct LstmGradLaunch {
  const float *rows;          // [B][R][T]
  const long long *n_valid;   // [B] or nullptr = R
  const float *target;        // [B]
  const unsigned char *mask;  // [B] or nullptr
  float *value;               // [B] or nullptr
  float *joint;               // [B][S + H] or nullptr
  float *partial;             // [chunks of this launch][D.floats]
  double *loss_part;          // [chunks of this launch]
  long long *count_part;      // [chunks of this launch]
  float grad_scale;
  int B, R;
  int chunk0;                 // the first chunk of this launch
  int SP;                     // states per pass: 4, 2 or 1 (read by the pass form only)
  ebc_lstmg::GradDims D;
};

struct LstmGradLds {
  float *X, *A1, *A2, *A3, *XI, *REC, *J, *M1, *M2, *M3, *DH, *DC, *ZERO, *OUT, *SEED;
  double *LOSS;
  int *LIVE, *N;
  int Tp, Jp, Hp, xis, RS;  // strides: X, J, a unit vector, XI (X's without mlp1), a step's record
};
// the floats of LDS for SP states at a time (SP = the chunk: the whole chunk at once); the arrays that are SP long are
// padded to 4 floats each, so that what follows them keeps its 16-byte (LOSS: 8-byte) alignment at every SP
__host__ __device__ inline size_t lstm_grad_lds_floats(const ebc_lstmg::GradDims &D, int R, int SP = EBC_LSTM_GRAD_CHUNK) {
  using namespace ebc_lstmg;
  const int Hp = pad4(D.H);
  const size_t slot = (size_t)pad4(D.T) + D.Op[L_M1A] + D.Op[L_M1B] + D.Op[L_M1C] + D.Op[L_M1D] + 4 * D.H + 3 * Hp;
  const size_t state = (size_t)pad4(D.K[L_MA]) + D.Op[L_MA] + D.Op[L_MB] + D.Op[L_MC] + 2 * Hp;
  return (size_t)SP * R * slot + SP * state + Hp + 4 * (size_t)pad4(SP) + pad4(2 * SP);
}
// the largest R at which SP states fit a workgroup's LDS (0: not even one row)
__host__ __device__ inline int lstm_grad_max_rows(const ebc_lstmg::GradDims &D, int SP = EBC_LSTM_GRAD_CHUNK) {
  int R = 0;
  while (R < 1024 && lstm_grad_lds_floats(D, R + 1, SP) * sizeof(float) <= EBC_LSTM_GRAD_LDS_BYTES) ++R;
  return R;
}
__device__ __forceinline__ LstmGradLds lstm_grad_lds(float *p, const ebc_lstmg::GradDims &D, int R, int SP) {
  using namespace ebc_lstmg;
  const int NR = SP * R, SPp = pad4(SP);
  LstmGradLds L;
  L.Tp = pad4(D.T), L.Jp = pad4(D.K[L_MA]), L.Hp = pad4(D.H), L.RS = 4 * D.H + 3 * L.Hp;
  L.X = p, p += NR * L.Tp;
  L.A1 = p, p += NR * D.Op[L_M1A];
  L.A2 = p, p += NR * D.Op[L_M1B];
  L.A3 = p, p += NR * D.Op[L_M1C];
  L.XI = D.two ? p : L.X, p += NR * D.Op[L_M1D];
  L.xis = D.two ? D.Op[L_M1D] : L.Tp;
  L.REC = p, p += NR * L.RS;
  L.J = p, p += SP * L.Jp;
  L.M1 = p, p += SP * D.Op[L_MA];
  L.M2 = p, p += SP * D.Op[L_MB];
  L.M3 = p, p += SP * D.Op[L_MC];
  L.DH = p, p += SP * L.Hp;
  L.DC = p, p += SP * L.Hp;
  L.ZERO = p, p += L.Hp;
  L.OUT = p, p += SPp;
  L.SEED = p, p += SPp;
  L.LOSS = reinterpret_cast<double *>(p), p += pad4(2 * SP);  // every array is a multiple of 4 floats long: so is every offset
  L.LIVE = reinterpret_cast<int *>(p), p += SPp;
  L.N = reinterpret_cast<int *>(p);
  return L;
}

constexpr int kLstmGradNT = 64 * EBC_LSTM_GRAD_WAVES;

// PASSES false: the whole chunk at once.  true: a.SP states at a time (see "Passes" above).
template <bool PASSES>
__global__ __launch_bounds__(kLstmGradNT) void lstm_grad_kernel(const float *__restrict__ P, const LstmGradLaunch a) {
  extern __shared__ float4 lstm_grad_lds4[];
  constexpr int C = EBC_LSTM_GRAD_CHUNK, NT = kLstmGradNT;
  using namespace ebc_lstmg;
  const GradDims &D = a.D;
  const int tid = threadIdx.x, R = a.R, T = D.T, S = D.S, I = D.I, H = D.H, H4 = 4 * D.H;
  const int SP = PASSES ? a.SP : C;
  const LstmGradLds L = lstm_grad_lds(reinterpret_cast<float *>(lstm_grad_lds4), D, R, SP);
  const int Tp = L.Tp, Jp = L.Jp, Hp = L.Hp, RS = L.RS, xis = L.xis;
  const int CO = H4, TCO = H4 + Hp, HO = H4 + 2 * Hp;  // c, tanh(c) and h in a step's record, after its 4 H gates
  const int O0 = D.Op[L_M1A], O1 = D.Op[L_M1B], O2 = D.Op[L_M1C], O4 = D.Op[L_MA], O5 = D.Op[L_MB], O6 = D.Op[L_MC];
  const long long chunk_at = ((long long)a.chunk0 + blockIdx.x) * C;
  const int chunk_n = a.B - chunk_at < C ? (int)(a.B - chunk_at) : C;  // states of this chunk, >= 1
  float *const part = a.partial + (size_t)blockIdx.x * D.floats;
  const float *const Wih = P + D.at_cell, *const Whh = Wih + (size_t)I * H4, *const Bih = Whh + (size_t)H * H4, *const Bhh = Bih + H4;
#define AT(l) (P + D.at[l])
#define GAT(l) (part + D.at[l])

  int at = 0;  // the pass's first state in the chunk
  do {
    const bool cont = PASSES && at > 0;
    const long long c0 = chunk_at + at;
    const int nc = chunk_n - at < SP ? chunk_n - at : SP;  // states of this pass, >= 1
    const int nq = nc * R;

    // ---- the states' row counts; the rows (zeros in the slots a state does not have: those are never read from memory)
    if (tid < Hp) L.ZERO[tid] = 0.0f;
    grad_load_rows<NT>(a, L, c0, nc, SP, T);
    int nmax = 0;
    for (int s = 0; s < nc; ++s) nmax = L.N[s] > nmax ? L.N[s] : nmax;
    __syncthreads();

    // ---- forward: mlp1
    if (D.two) {
      grad_layer<NT, true>(AT(L_M1A), T, 0, D.O[L_M1A], O0, L.X, Tp, nullptr, 0, R, L.A1, O0, nq);
      __syncthreads();
      grad_layer<NT, true>(AT(L_M1B), D.K[L_M1B], 0, D.O[L_M1B], O1, L.A1, O0, nullptr, 0, R, L.A2, O1, nq);
      __syncthreads();
      grad_layer<NT, true>(AT(L_M1C), D.K[L_M1C], 0, D.O[L_M1C], O2, L.A2, O1, nullptr, 0, R, L.A3, O2, nq);
      __syncthreads();
      grad_layer<NT, false>(AT(L_M1D), D.K[L_M1D], 0, I, xis, L.A3, O2, nullptr, 0, R, L.XI, xis, nq);
      __syncthreads();
    }

    // ---- forward: the recurrence, a step at a time
    const int pairs = (nc + 1) / 2;
    for (int t = 0; t < nmax; ++t) {
      for (int idx = tid; idx < pairs * H4; idx += NT) {
        const int pair = idx / H4, q = idx - pair * H4, s0 = 2 * pair, s1 = s0 + 1 < nc ? s0 + 1 : s0;
        const float *x0 = L.XI + (size_t)(s0 * R + t) * xis, *x1 = L.XI + (size_t)(s1 * R + t) * xis;
        const float *h0 = t ? L.REC + (size_t)(s0 * R + t - 1) * RS + HO : L.ZERO, *h1 = t ? L.REC + (size_t)(s1 * R + t - 1) * RS + HO : L.ZERO;
        float acc0 = gate_bias(Bih[q], Bhh[q]), acc1 = acc0;
        for (int k = 0; k < I; ++k) {
          const float w = Wih[(size_t)k * H4 + q];
          acc0 = gate_chain(w, x0[k], acc0);
          acc1 = gate_chain(w, x1[k], acc1);
        }
        for (int k = 0; k < H; ++k) {
          const float w = Whh[(size_t)k * H4 + q];
          acc0 = gate_chain(w, h0[k], acc0);
          acc1 = gate_chain(w, h1[k], acc1);
        }
        if (t < L.N[s0]) L.REC[(size_t)(s0 * R + t) * RS + q] = acc0;
        if (s1 != s0 && t < L.N[s1]) L.REC[(size_t)(s1 * R + t) * RS + q] = acc1;
      }
      __syncthreads();
      for (int idx = tid; idx < nc * H; idx += NT) {
        const int s = idx / H, u = idx - s * H;
        if (t >= L.N[s]) continue;
        float *rec = L.REC + (size_t)(s * R + t) * RS;
        const float c_prev = t ? rec[CO + u - RS] : 0.0f;
        cell_forward(rec[u], rec[H + u], rec[2 * H + u], rec[3 * H + u], c_prev, rec[u], rec[H + u], rec[2 * H + u], rec[3 * H + u], rec[CO + u],
                     rec[TCO + u], rec[HO + u]);
      }
      __syncthreads();
    }

    // ---- the joint vector: the self state of row 0 and h of the state's last step
    for (int i = tid; i < nc * (S + H); i += NT) {
      const int s = i / (S + H), k = i - s * (S + H), n = L.N[s];
      const float v = n < 1 ? 0.0f : (k < S ? L.X[(s * R) * Tp + k] : L.REC[(size_t)(s * R + n - 1) * RS + HO + (k - S)]);
      L.J[s * Jp + k] = v;
      if (a.joint) a.joint[(size_t)(c0 + s) * (S + H) + k] = n < 1 ? 0.0f : canon(v);
    }
    __syncthreads();
    // ---- mlp
    grad_layer<NT, true>(AT(L_MA), S + H, 0, D.O[L_MA], O4, L.J, Jp, nullptr, 0, R, L.M1, O4, nc);
    __syncthreads();
    grad_layer<NT, true>(AT(L_MB), D.K[L_MB], 0, D.O[L_MB], O5, L.M1, O4, nullptr, 0, R, L.M2, O5, nc);
    __syncthreads();
    grad_layer<NT, true>(AT(L_MC), D.K[L_MC], 0, D.O[L_MC], O6, L.M2, O5, nullptr, 0, R, L.M3, O6, nc);
    __syncthreads();
    grad_layer<NT, false>(AT(L_MD), D.K[L_MD], 0, 1, D.Op[L_MD], L.M3, O6, nullptr, 0, R, L.OUT, 1, nc);
    __syncthreads();

    // ---- the values and the seeds, a thread per state; the chunk's loss in state order: thread 0's
    grad_seed(a, L, c0, nc, SP, cont);

    // ---- backward: mlp
    grad_dw<NT>(GAT(L_MD), D.K[L_MD], 0, 1, D.Op[L_MD], L.SEED, 1, L.M3, O6, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_MD), 0, D.K[L_MD], 1, D.Op[L_MD], L.SEED, 1, L.M3, O6, R, nc, L.N, L.LIVE, false, false);
    __syncthreads();
    grad_dw<NT>(GAT(L_MC), D.K[L_MC], 0, D.O[L_MC], O6, L.M3, O6, L.M2, O5, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_MC), 0, D.K[L_MC], D.O[L_MC], O6, L.M3, O6, L.M2, O5, R, nc, L.N, L.LIVE, false, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_MB), D.K[L_MB], 0, D.O[L_MB], O5, L.M2, O5, L.M1, O4, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    __syncthreads();
    grad_dx<NT, true>(AT(L_MB), 0, D.K[L_MB], D.O[L_MB], O5, L.M2, O5, L.M1, O4, R, nc, L.N, L.LIVE, false, true);
    __syncthreads();
    grad_dw<NT>(GAT(L_MA), S + H, 0, D.O[L_MA], O4, L.M1, O4, L.J, Jp, nullptr, 0, R, nc, L.N, L.LIVE, false, cont);
    grad_dx<NT, false>(AT(L_MA), S, S + H, D.O[L_MA], O4, L.M1, O4, L.DH, Hp, R, nc, L.N, L.LIVE, false, true);  // dh of the last step
    for (int i = tid; i < nc * H; i += NT) L.DC[(i / H) * Hp + (i % H)] = 0.0f;
    __syncthreads();

    // ---- backward through time: the gates become their deltas
    for (int t = nmax - 1; t >= 0; --t) {
      for (int idx = tid; idx < nc * H; idx += NT) {
        const int s = idx / H, u = idx - s * H;
        if (!L.LIVE[s] || t >= L.N[s]) continue;
        float *rec = L.REC + (size_t)(s * R + t) * RS;
        const float c_prev = t ? rec[CO + u - RS] : 0.0f;
        cell_back(L.DH[s * Hp + u], L.DC[s * Hp + u], rec[u], rec[H + u], rec[2 * H + u], rec[3 * H + u], rec[TCO + u], c_prev, rec[u], rec[H + u],
                  rec[2 * H + u], rec[3 * H + u], L.DC[s * Hp + u]);
      }
      __syncthreads();
      if (t == 0) break;
      for (int idx = tid; idx < nc * H; idx += NT) {
        const int k = idx / nc, s = idx - k * nc;
        if (!L.LIVE[s] || t >= L.N[s]) continue;
        L.DH[s * Hp + k] = grad_dot(Whh + (size_t)k * H4, L.REC + (size_t)(s * R + t) * RS, H4, true);
      }
      __syncthreads();
    }

    // ---- the cell's weights: w_ih [I][4 H] | w_hh [H][4 H] | b_ih | b_hh are (I + H + 2) rows of 4 H in the image
    for (int idx = tid; idx < (I + H + 2) * H4; idx += NT) {
      const int k = idx / H4, q = idx - k * H4;
      float acc = cont ? part[D.at_cell + idx] : 0.0f;
      for (int s = 0; s < nc; ++s) {
        if (!L.LIVE[s]) continue;
        const int n = L.N[s];
        const float *rec = L.REC + (size_t)(s * R) * RS;
        if (k < I) {
          for (int t = 0; t < n; ++t) acc = chain(rec[(size_t)t * RS + q], L.XI[(size_t)(s * R + t) * xis + k], acc);
        } else if (k < I + H) {
          for (int t = 0; t < n; ++t) acc = chain(rec[(size_t)t * RS + q], t ? rec[(size_t)(t - 1) * RS + HO + (k - I)] : 0.0f, acc);
        } else {
          for (int t = 0; t < n; ++t) acc = acc + rec[(size_t)t * RS + q];
        }
      }
      part[D.at_cell + idx] = acc;
    }
    if (D.two) {
      // ---- mlp1: xi becomes its delta (the cell's dW above has read it)
      __syncthreads();
      grad_dx<NT, false>(Wih, 0, I, H4, H4, L.REC, RS, L.XI, xis, R, nc, L.N, L.LIVE, true, true);
      __syncthreads();
      grad_dw<NT>(GAT(L_M1D), D.K[L_M1D], 0, I, xis, L.XI, xis, L.A3, O2, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
      __syncthreads();
      grad_dx<NT, true>(AT(L_M1D), 0, D.K[L_M1D], I, xis, L.XI, xis, L.A3, O2, R, nc, L.N, L.LIVE, true, true);
      __syncthreads();
      grad_dw<NT>(GAT(L_M1C), D.K[L_M1C], 0, D.O[L_M1C], O2, L.A3, O2, L.A2, O1, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
      __syncthreads();
      grad_dx<NT, true>(AT(L_M1C), 0, D.K[L_M1C], D.O[L_M1C], O2, L.A3, O2, L.A2, O1, R, nc, L.N, L.LIVE, true, true);
      __syncthreads();
      grad_dw<NT>(GAT(L_M1B), D.K[L_M1B], 0, D.O[L_M1B], O1, L.A2, O1, L.A1, O0, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
      __syncthreads();
      grad_dx<NT, true>(AT(L_M1B), 0, D.K[L_M1B], D.O[L_M1B], O1, L.A2, O1, L.A1, O0, R, nc, L.N, L.LIVE, true, true);
      __syncthreads();
      grad_dw<NT>(GAT(L_M1A), T, 0, D.O[L_M1A], O0, L.A1, O0, L.X, Tp, nullptr, 0, R, nc, L.N, L.LIVE, true, cont);
    }
    if (PASSES) __syncthreads();  // the next pass's forward overwrites what this pass's dW reads
  } while (PASSES && (at += SP) < chunk_n);
#undef AT
#undef GAT
}

}  // namespace ebc
