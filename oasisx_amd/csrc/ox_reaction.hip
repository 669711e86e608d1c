// Reacting scalars: stiff mass-action kinetics, split from the transport step.
//
//   r_j  = k_j(x) [exp(-Ta_j / c_T)] prod_s c_s^o_js          the rate of reaction j at a dof
//   f_s  = sum_j nu_sj r_j                                    the source of species s
//
// k_scalar_react     `substeps` steps of ROS2 (Verwer, Spee, Blom, Hundsdorfer 1999: second order, L-stable, one LU per
//                    step, the analytic Jacobian) per dof, with g = 1 + 1/sqrt(2), W = I - (g h) J(y):
//                      W k1 = f(y);   W k2 = f(y + h k1) - 2 k1;   y <- (y + (1.5 h) k1) + (0.5 h) k2
//                    One lane per dof, one instantiation per number of species S.  A lane reads its S values once (from
//                    columns of interleaved (n, nc) blocks, nc per species), keeps y, f, W, k1, k2 in registers over all
//                    substeps and writes S values once (to one or two blocks).  Every index into a register array is a
//                    compile-time constant: the loops over species are fully unrolled, rows are exchanged through selects
//                    and the pivots are S named integers.  The loop over the reactions is a run-time loop: the network
//                    tables live in the kernel arguments, j is lane-uniform, the loads are scalar.  A per-dof rate
//                    coefficient is read where it is used (three times per substep, from the cache after the first).
//                    No LDS, no atomics, no scratch.
// k_reaction_rates   the same rate function, r_j to rates[j][i].
//
// The orders are integers 0..3 formed by repeated multiplication (c, c c, (c c) c): no pow, and nothing is divided by a
// concentration; the derivative lowers one factor's order (1, 2 c, 3 (c c)).  Only the Arrhenius factor divides, by its
// temperature.
#include "ox_kernels.h"
#include <cmath>

namespace {

template <int S>
struct ReactSpecies {
  ox_react_species s[S];
};

// c^o and o c^(o-1) for the lane-uniform order o in 0..3
__device__ __forceinline__ void react_power(int o, double c, double &p, double &q) {
  const double c2 = c * c;
  p = o == 0 ? 1.0 : o == 1 ? c : o == 2 ? c2 : c2 * c;
  q = o == 0 ? 0.0 : o == 1 ? 1.0 : o == 2 ? 2.0 * c : 3.0 * c2;
}

// Reaction j at the state y: ka = k_j a_j, r = r_j, p / q the powers and their derivatives, cT the Arrhenius temperature.
template <int S>
__device__ __forceinline__ void react_rate(const ox_react_net &N, int j, int64_t i, const double (&y)[S], double &ka,
                                           double &r, double (&p)[S], double (&q)[S], double &cT) {
  const double *kd = N.kdof[j];
  ka = kd ? kd[i] : N.k[j];
  const int a = N.arr[j];
  cT = 0.0;
  if (a >= 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) cT = a == s ? y[s] : cT;
    ka = ka * exp(-N.Ta[j] / cT);
  }
  r = ka;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    react_power(N.order[j][s], y[s], p[s], q[s]);
    r = r * p[s];
  }
}

// f(y) and, with JAC, J(y) = f'(y): reactions ascending, from 0.
template <int S, bool JAC>
__device__ __forceinline__ void react_rhs(const ox_react_net &N, int64_t i, const double (&y)[S], double (&f)[S],
                                          double (&J)[S][S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    f[s] = 0.0;
    if constexpr (JAC) {
#pragma unroll
      for (int t = 0; t < S; ++t) J[s][t] = 0.0;
    }
  }
  for (int j = 0; j < N.R; ++j) {
    double ka, r, cT, p[S], q[S];
    react_rate<S>(N, j, i, y, ka, r, p, q, cT);
#pragma unroll
    for (int s = 0; s < S; ++s) f[s] = f[s] + N.nu[s][j] * r;
    if constexpr (JAC) {
      const int a = N.arr[j];
      const double da = a >= 0 ? (r * N.Ta[j]) / (cT * cT) : 0.0;
#pragma unroll
      for (int t = 0; t < S; ++t) {
        double d = ka;
#pragma unroll
        for (int s = 0; s < S; ++s) d = d * (s == t ? q[s] : p[s]);
        d = a == t ? d + da : d;
#pragma unroll
        for (int s = 0; s < S; ++s) J[s][t] = J[s][t] + N.nu[s][j] * d;
      }
    }
  }
}

// W = P^T L U in place: partial pivoting (largest |.| of the column at or below the diagonal, ties to the lower row), the
// multipliers below the diagonal, the RECIPROCAL of the pivot on it.  piv[c]: the row exchanged with row c.
template <int S>
__device__ __forceinline__ void react_lu(double (&W)[S][S], int (&piv)[S]) {
#pragma unroll
  for (int c = 0; c < S; ++c) {
    int pr = c;
    double best = fabs(W[c][c]);
#pragma unroll
    for (int r = c + 1; r < S; ++r) {
      const double v = fabs(W[r][c]);
      const bool g = v > best;
      pr = g ? r : pr;
      best = g ? v : best;
    }
    piv[c] = pr;
#pragma unroll
    for (int r = c + 1; r < S; ++r) {
      const bool sw = pr == r;
#pragma unroll
      for (int t = 0; t < S; ++t) {
        const double a = W[c][t], b = W[r][t];
        W[c][t] = sw ? b : a;
        W[r][t] = sw ? a : b;
      }
    }
    const double inv = 1.0 / W[c][c];
    W[c][c] = inv;
#pragma unroll
    for (int r = c + 1; r < S; ++r) {
      const double m = W[r][c] * inv;
      W[r][c] = m;
#pragma unroll
      for (int t = c + 1; t < S; ++t) W[r][t] = W[r][t] - m * W[c][t];
    }
  }
}

// x <- W^-1 x with the factors of react_lu: the exchanges, L (unit diagonal) forwards, U backwards (columns ascending).
template <int S>
__device__ __forceinline__ void react_lu_solve(const double (&W)[S][S], const int (&piv)[S], double (&x)[S]) {
#pragma unroll
  for (int c = 0; c < S; ++c) {
#pragma unroll
    for (int r = c + 1; r < S; ++r) {
      const bool sw = piv[c] == r;
      const double a = x[c], b = x[r];
      x[c] = sw ? b : a;
      x[r] = sw ? a : b;
    }
#pragma unroll
    for (int r = c + 1; r < S; ++r) x[r] = x[r] - W[r][c] * x[c];
  }
#pragma unroll
  for (int c = S - 1; c >= 0; --c) {
    double acc = x[c];
#pragma unroll
    for (int t = c + 1; t < S; ++t) acc = acc - W[c][t] * x[t];
    x[c] = acc * W[c][c];
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_scalar_react(ox_react_net N, ReactSpecies<S> A, int64_t n, double h, double gh,
                                                      int substeps) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double y[S], y0[S];
#pragma unroll
  for (int s = 0; s < S; ++s) y0[s] = y[s] = A.s[s].src[(size_t)i * A.s[s].nc + A.s[s].col];
  const double h15 = 1.5 * h, h05 = 0.5 * h;
  for (int m = 0; m < substeps; ++m) {
    double f[S], W[S][S], k1[S], k2[S], y1[S];
    int piv[S];
    react_rhs<S, true>(N, i, y, k1, W);
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < S; ++t) W[s][t] = (s == t ? 1.0 : 0.0) - gh * W[s][t];
    react_lu<S>(W, piv);
    react_lu_solve<S>(W, piv, k1);
#pragma unroll
    for (int s = 0; s < S; ++s) y1[s] = y[s] + h * k1[s];
    react_rhs<S, false>(N, i, y1, f, W);
#pragma unroll
    for (int s = 0; s < S; ++s) k2[s] = f[s] - 2.0 * k1[s];
    react_lu_solve<S>(W, piv, k2);
#pragma unroll
    for (int s = 0; s < S; ++s) y[s] = (y[s] + h15 * k1[s]) + h05 * k2[s];
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uint8_t *held = A.s[s].held;
    const double v = (held && held[i]) ? y0[s] : y[s];
    const size_t k = (size_t)i * A.s[s].nc + A.s[s].col;
    A.s[s].out[k] = v;
    if (A.s[s].out2) A.s[s].out2[k] = v;
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_reaction_rates(ox_react_net N, ReactSpecies<S> A, int64_t n,
                                                        double *__restrict__ rates) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double y[S];
#pragma unroll
  for (int s = 0; s < S; ++s) y[s] = A.s[s].src[(size_t)i * A.s[s].nc + A.s[s].col];
  for (int j = 0; j < N.R; ++j) {
    double ka, r, cT, p[S], q[S];
    react_rate<S>(N, j, i, y, ka, r, p, q, cT);
    rates[(size_t)j * n + i] = r;
  }
}

template <int S>
int launch_react(const ox_react_net *net, const ox_react_species *sp, int64_t n, double H, int substeps, double *rates,
                 hipStream_t st) {
  ReactSpecies<S> A;
  for (int s = 0; s < S; ++s) A.s[s] = sp[s];
  const unsigned nblk = (unsigned)((n + 255) / 256);
  const long long key = 100LL * S + net->R;
  if (rates) {
    if (ox_prof_on) ox_prof_start(OX_TAG_REACTION_RATES, st, key);
    hipLaunchKernelGGL((k_reaction_rates<S>), dim3(nblk), dim3(256), 0, st, *net, A, n, rates);
  } else {
    const double h = H / substeps;
    const double gh = 1.7071067811865475 * h;  // 1 + 1/sqrt(2)
    if (ox_prof_on) ox_prof_start(OX_TAG_SCALAR_REACT, st, key);
    hipLaunchKernelGGL((k_scalar_react<S>), dim3(nblk), dim3(256), 0, st, *net, A, n, h, gh, substeps);
  }
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

int react_check(const char *who, const ox_react_net *net, const ox_react_species *sp, int64_t n, bool writes) {
  if (!net || !sp) OX_FAIL("%s: null argument", who);
  if (net->S < 1 || net->S > OX_REACT_MAXS) OX_FAIL("%s: %d species (1..%d)", who, (int)net->S, OX_REACT_MAXS);
  if (net->R < 1 || net->R > OX_REACT_MAXR) OX_FAIL("%s: %d reactions (1..%d)", who, (int)net->R, OX_REACT_MAXR);
  if (n < 0 || n > (int64_t)0x7fffffff * 256) OX_FAIL("%s: n=%lld", who, (long long)n);
  for (int j = 0; j < net->R; ++j) {
    if (net->arr[j] < -1 || net->arr[j] >= net->S) OX_FAIL("%s: reaction %d: Arrhenius species %d", who, j, (int)net->arr[j]);
    for (int s = 0; s < net->S; ++s)
      if (net->order[j][s] < 0 || net->order[j][s] > 3)
        OX_FAIL("%s: reaction %d: order %d of species %d (0..3)", who, j, (int)net->order[j][s], s);
  }
  for (int s = 0; s < net->S; ++s) {
    if (!sp[s].src || (writes && !sp[s].out)) OX_FAIL("%s: species %d has no block", who, s);
    if (sp[s].nc < 1 || sp[s].col < 0 || sp[s].col >= sp[s].nc)
      OX_FAIL("%s: species %d: column %d of %d", who, s, (int)sp[s].col, (int)sp[s].nc);
  }
  return 0;
}

int react_dispatch(const ox_react_net *net, const ox_react_species *sp, int64_t n, double H, int substeps, double *rates,
                   hipStream_t st) {
  switch (net->S) {
    case 1: return launch_react<1>(net, sp, n, H, substeps, rates, st);
    case 2: return launch_react<2>(net, sp, n, H, substeps, rates, st);
    case 3: return launch_react<3>(net, sp, n, H, substeps, rates, st);
    case 4: return launch_react<4>(net, sp, n, H, substeps, rates, st);
    case 5: return launch_react<5>(net, sp, n, H, substeps, rates, st);
    default: return launch_react<6>(net, sp, n, H, substeps, rates, st);
  }
}

}  // namespace

extern "C" int ox_scalar_react(const ox_react_net *net, const ox_react_species *species, int64_t n, double H, int substeps,
                               void *stream) {
  if (react_check("ox_scalar_react", net, species, n, true)) return -1;
  if (substeps < 1) OX_FAIL("ox_scalar_react: substeps=%d", substeps);
  if (n == 0) return 0;
  return react_dispatch(net, species, n, H, substeps, nullptr, ox_stream(stream));
}

extern "C" int ox_reaction_rates(const ox_react_net *net, const ox_react_species *species, int64_t n, double *rates,
                                 void *stream) {
  if (react_check("ox_reaction_rates", net, species, n, false)) return -1;
  if (!rates) OX_FAIL("ox_reaction_rates: null argument");
  if (n == 0) return 0;
  return react_dispatch(net, species, n, 0.0, 1, rates, ox_stream(stream));
}
