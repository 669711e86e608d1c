// Flow diagnostics and running statistics.  Nothing here writes a solver field or touches a matrix.
//
// ox_flow_cells: one lane per cell, in kernel cell order -- the streams of k_cell_viscosity (the cell's dof list, its
// geometry record, the gathered ND x GDIM coefficients) plus a quadrature loop.  With g = grad u (g[d][k] = du_d/dx_k),
// S = sym g, W = skew g, omega = curl u:
//
//   cell integrals (exact for the element)                       centroid quantities (fields, optional)
//     vol     = |cell| = |det J| / gdim!                           cfl   = dt max_a |u(x_c) . grad lambda_a|
//     ke      = 1/2 int |u|^2      (mass table, degree 2 DEG)      shear = sqrt(2 S:S)       (gd of the viscosity laws)
//     strain2 = int 2 S:S          (rule of degree 2 (DEG - 1))    divc  = tr g
//     diss    = (nu + nut_c) strain2                               q     = 1/2 (W:W - S:S)
//     ens     = 1/2 int |omega|^2                                  omega: g[1][0] - g[0][1]  |  the three of curl u
//     div2    = int (div u)^2
//     div1    = int div u
//
// ke contracts the dofs with the mean mass matrix of the element (compile-time constants, zero entries cost nothing);
// the gradient forms are summed on a positive-weight rule whose tables sit in __constant__ memory and are read with a
// lane-uniform point index (scalar loads).  Per 256-lane block the seven sums and max cfl go to partials[block][8]
// through a fixed shuffle / LDS tree: no atomics, equal inputs give equal bits.  The maximum PROPAGATES NaN (fmax would
// drop it): a run that has blown up shows NaN, not the largest finite value.
//
// ox_flow_reduce: one block, lane-strided over the partial rows in a fixed order, the same tree, ring[slot][0..7].
//
// ox_stats_accumulate: West's (1979) weighted incremental update of mean and upper-triangular covariance sums per dof,
// one thread per dof (pure streaming, 16-byte accesses where the interleaved layout allows, no atomics).
//
// ox_profile_cells / ox_profile_update: the moments of a joint vector q over the cells of a bin (a
// slab of a homogeneous direction), exact for the element through the same mean mass matrix, taken about a per-bin shift;
// cells reach their bin through a sorted permutation cut into chunks of <= 256 that never cross a bin, one block per
// chunk, one wave per bin for the merge into the running mean and second moment.  No atomics either.
#define OX_DIAG_RULE_QUAL __constant__
#include "fe_tables_d.h"
#include "ox_element.h"
#include <cmath>

namespace {

// Sizes and tables particular to the diagnostics: the centroid values and the mean mass matrix of the basis
// (compile-time constants) and the rule of degree 2 (DEG - 1), read at run time from __constant__ memory.
template <int GDIM, int DEG>
struct Diag {
  static constexpr int NF = 4 + (GDIM == 2 ? 1 : 3);
  static constexpr int B0 = DEG == 3 ? 1 : 0;  // (P3: the basis is a polynomial of lambda_1..d, column 0 is zero)
  __host__ __device__ static constexpr int nq() { OX_FE_PICK(GDIM, DEG, OX_NQD, ); }
  __host__ __device__ static constexpr double phic(int i) { OX_FE_PICK(GDIM, DEG, OX_PHIC, [i]); }
  __host__ __device__ static constexpr double mass(int i, int j) { OX_FE_PICK(GDIM, DEG, OX_MASSD, [i][j]); }
  __device__ static const double *qw() { OX_FE_PICK(GDIM, DEG, OX_QWD, ); }
  __device__ static const double *dphiq() { OX_FE_PICK(GDIM, DEG, OX_DPHID, [0][0]); }  // [q][i][b], b = 0..GDIM
};

// max that keeps a NaN (and, like fmax, prefers neither sign of zero: the operands here are >= 0 or NaN)
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__device__ __forceinline__ double wave_nan_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_down(v, off, 64));
  return v;  // valid in lane 0
}

// The seven sums and the maximum of a 256-lane block, valid in thread 0: wave shuffles, then the four wave results in
// wave order.  lds: [4 * 8].
__device__ __forceinline__ void block_reduce8(double (&v)[7], double &m, double *lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const double s = ox_wave_sum(v[i]);
    if (lane == 0) lds[wave * 8 + i] = s;
  }
  const double mm = wave_nan_max(m);
  if (lane == 0) lds[wave * 8 + 7] = mm;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] = lds[i] + lds[8 + i] + lds[16 + i] + lds[24 + i];
    m = nan_max(nan_max(lds[7], lds[15]), nan_max(lds[23], lds[31]));
  }
}

// S:S, |omega|^2 (omega: the GDIM == 2 ? 1 : 3 components of curl u) and tr g
template <int GDIM>
__device__ __forceinline__ void invariants(const double (&g)[GDIM][GDIM], double &ss, double (&om)[GDIM == 2 ? 1 : 3],
                                           double &om2, double &tr) {
  ss = ox_sym_sq<GDIM>(g);
  if constexpr (GDIM == 2) {
    om[0] = g[1][0] - g[0][1];
    om2 = om[0] * om[0];
    tr = g[0][0] + g[1][1];
  } else {
    om[0] = g[2][1] - g[1][2];
    om[1] = g[0][2] - g[2][0];
    om[2] = g[1][0] - g[0][1];
    om2 = fma(om[2], om[2], fma(om[1], om[1], om[0] * om[0]));
    tr = g[0][0] + g[1][1] + g[2][2];
  }
}

template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_flow_cells(ox_cells cells, const int32_t *__restrict__ cell_dofs,
                                                    const double *__restrict__ u, const double *__restrict__ nut, double dt,
                                                    double nu, double *__restrict__ fields, double *__restrict__ cint,
                                                    double *__restrict__ partials) {
  using E = Diag<GDIM, DEG>;
  constexpr int ND = ox_nd(GDIM, DEG), NF = E::NF, B0 = E::B0;
  __shared__ double lds[32];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) v[i] = 0.0;
  double cfl = 0.0;
  if (e < cells.n_cells) {
    // round 1: the cell's dofs and geometry (both indexed by e); round 2: the coefficient gathers
    int32_t dd[ND];
    ox_load_dofs<ND>(cell_dofs, e, dd);
    double G[GDIM + 1][GDIM], adet;
    ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
    double uc[ND][GDIM];
    ox_gather<ND, GDIM>(dd, u, uc);
    const double vol = ox_cell_volume<GDIM>(adet);

    // ---- ke = 1/2 |cell| sum_d u_d^T M u_d, M the mean mass matrix
    double k2 = 0.0;
#pragma unroll
    for (int d = 0; d < GDIM; ++d)
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < ND; ++j)
          if (E::mass(i, j) != 0.0) r = fma(E::mass(i, j), uc[j][d], r);
        k2 = fma(uc[i][d], r, k2);
      }

    // ---- the gradient forms on the rule of degree 2 (DEG - 1): weights sum to 1, the sums are cell MEANS
    double s2 = 0.0, en = 0.0, d2 = 0.0, d1 = 0.0;
    const double *__restrict__ wq = E::qw();
    const double *__restrict__ dq = E::dphiq();
#pragma unroll 1
    for (int q = 0; q < E::nq(); ++q) {
      double t[GDIM][GDIM + 1];
#pragma unroll
      for (int d = 0; d < GDIM; ++d)
#pragma unroll
        for (int b = 0; b <= GDIM; ++b) t[d][b] = 0.0;
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int b = B0; b <= GDIM; ++b) {
          const double c = dq[(q * ND + i) * (GDIM + 1) + b];
#pragma unroll
          for (int d = 0; d < GDIM; ++d) t[d][b] = fma(uc[i][d], c, t[d][b]);
        }
      double g[GDIM][GDIM], om[GDIM == 2 ? 1 : 3], ss, om2, tr;
      ox_grad_from_t<GDIM>(t, G, g, B0);
      invariants<GDIM>(g, ss, om, om2, tr);
      const double w = wq[q];
      s2 = fma(w, 2.0 * ss, s2);
      en = fma(w, om2, en);
      d2 = fma(w, tr * tr, d2);
      d1 = fma(w, tr, d1);
    }
    v[0] = vol;
    v[1] = (0.5 * vol) * k2;
    v[2] = vol * s2;
    v[3] = (nut ? nu + nut[e] : nu) * v[2];
    v[4] = (0.5 * vol) * en;
    v[5] = vol * d2;
    v[6] = vol * d1;
    if (cint) {
#pragma unroll
      for (int i = 0; i < 7; ++i) cint[(size_t)e * 7 + i] = v[i];
    }

    // ---- the centroid: grad u as k_cell_viscosity forms it, u(x_c) for the CFL number
    double t[GDIM][GDIM + 1] = {}, ucen[GDIM] = {};
    ox_contract<GDIM, ND>(uc, ox_dphic<GDIM, DEG>(), t);
#pragma unroll
    for (int i = 0; i < ND; ++i)
      if (E::phic(i) != 0.0) {
#pragma unroll
        for (int d = 0; d < GDIM; ++d) ucen[d] = fma(uc[i][d], E::phic(i), ucen[d]);
      }
    double m = 0.0;
#pragma unroll
    for (int a = 0; a <= GDIM; ++a) {
      double r = 0.0;
#pragma unroll
      for (int d = 0; d < GDIM; ++d) r = fma(ucen[d], G[a][d], r);
      m = nan_max(m, fabs(r));
    }
    cfl = dt * m;
    if (fields) {
      double g[GDIM][GDIM], om[GDIM == 2 ? 1 : 3], ss, om2, tr;
      ox_grad_from_t<GDIM>(t, G, g);
      invariants<GDIM>(g, ss, om, om2, tr);
      double ww = 0.0;  // W:W
#pragma unroll
      for (int d = 0; d < GDIM; ++d)
#pragma unroll
        for (int k = 0; k < GDIM; ++k) {
          const double a = 0.5 * (g[d][k] - g[k][d]);
          ww = fma(a, a, ww);
        }
      double *__restrict__ f = fields + (size_t)e * NF;
      f[0] = cfl;
      f[1] = sqrt(2.0 * ss);
      f[2] = tr;
      f[3] = 0.5 * (ww - ss);
#pragma unroll
      for (int c = 0; c < NF - 4; ++c) f[4 + c] = om[c];
    }
  }
  block_reduce8(v, cfl, lds);
  if (threadIdx.x == 0) {
    double *__restrict__ p = partials + (size_t)blockIdx.x * 8;
#pragma unroll
    for (int i = 0; i < 7; ++i) p[i] = v[i];
    p[7] = cfl;
  }
}

__global__ __launch_bounds__(256) void k_flow_reduce(int64_t n_blocks, const double *__restrict__ partials,
                                                     double *__restrict__ row) {
  __shared__ double lds[32];
  double v[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) v[i] = 0.0;
  double m = 0.0;
  for (int64_t r = threadIdx.x; r < n_blocks; r += 256) {
    const double *__restrict__ p = partials + (size_t)r * 8;
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] += p[i];
    m = nan_max(m, p[7]);
  }
  block_reduce8(v, m, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) row[i] = v[i];
    row[7] = m;
  }
}

// West's update of one dof: a = w / W', b = W a = w W / W'
template <int NC>
__device__ __forceinline__ void west(const double (&x)[NC], double a, double b, double (&mean)[NC],
                                     double (&cov)[NC * (NC + 1) / 2]) {
  double dl[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) dl[c] = x[c] - mean[c];
#pragma unroll
  for (int c = 0; c < NC; ++c) mean[c] = fma(a, dl[c], mean[c]);
  int k = 0;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int j = i; j < NC; ++j, ++k) cov[k] = fma(b * dl[i], dl[j], cov[k]);
}

// One thread per dof.  VEC: x is dense (ldx == NC) and every pointer is 16-byte aligned -- the 16-byte-aligned groups of
// the interleaved rows move as double2 (NC = 2: x and mean; NC = 3: cov, 48 B per dof; NC = 1: two dofs per thread).
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void k_stats(int64_t n, const double *__restrict__ x, int64_t ldx, double a, double b,
                                               int first, double *__restrict__ mean, double *__restrict__ cov) {
  constexpr int NV = NC * (NC + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (NC == 1 && VEC) {
    const int64_t np = n >> 1;
    if (i < np) {
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      double2 mv = reinterpret_cast<double2 *>(mean)[i], cv = reinterpret_cast<double2 *>(cov)[i];
      if (first) {
        mv = xv;
        cv = make_double2(0.0, 0.0);
      } else {
        double xs[1] = {xv.x}, ms[1] = {mv.x}, cs[1] = {cv.x};
        west<1>(xs, a, b, ms, cs);
        mv.x = ms[0], cv.x = cs[0];
        xs[0] = xv.y, ms[0] = mv.y, cs[0] = cv.y;
        west<1>(xs, a, b, ms, cs);
        mv.y = ms[0], cv.y = cs[0];
      }
      reinterpret_cast<double2 *>(mean)[i] = mv;
      reinterpret_cast<double2 *>(cov)[i] = cv;
    } else if (i == np && (n & 1)) {
      const int64_t k = n - 1;
      if (first) {
        mean[k] = x[k];
        cov[k] = 0.0;
      } else {
        double xs[1] = {x[k]}, ms[1] = {mean[k]}, cs[1] = {cov[k]};
        west<1>(xs, a, b, ms, cs);
        mean[k] = ms[0], cov[k] = cs[0];
      }
    }
  } else {
    if (i >= n) return;
    double xs[NC], ms[NC], cs[NV];
    if constexpr (NC == 2 && VEC) {
      const double2 xv = reinterpret_cast<const double2 *>(x)[i];
      xs[0] = xv.x, xs[1] = xv.y;
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) xs[c] = x[(size_t)i * ldx + c];
    }
    if (first) {
#pragma unroll
      for (int c = 0; c < NC; ++c) ms[c] = xs[c];
#pragma unroll
      for (int k = 0; k < NV; ++k) cs[k] = 0.0;
    } else {
      if constexpr (NC == 2 && VEC) {
        const double2 mv = reinterpret_cast<const double2 *>(mean)[i];
        ms[0] = mv.x, ms[1] = mv.y;
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) ms[c] = mean[(size_t)i * NC + c];
      }
      if constexpr (NC == 3 && VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double2 cv = reinterpret_cast<const double2 *>(cov)[(size_t)i * 3 + k];
          cs[2 * k] = cv.x, cs[2 * k + 1] = cv.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) cs[k] = cov[(size_t)i * NV + k];
      }
      west<NC>(xs, a, b, ms, cs);
    }
    if constexpr (NC == 2 && VEC) {
      reinterpret_cast<double2 *>(mean)[i] = make_double2(ms[0], ms[1]);
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) mean[(size_t)i * NC + c] = ms[c];
    }
    if constexpr (NC == 3 && VEC) {
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<double2 *>(cov)[(size_t)i * 3 + k] = make_double2(cs[2 * k], cs[2 * k + 1]);
    } else {
#pragma unroll
      for (int k = 0; k < NV; ++k) cov[(size_t)i * NV + k] = cs[k];
    }
  }
}

// ---- slab-averaged statistics -----------------------------------------------------------------
// The joint vector q of a group has NQ components: the first NC0 = (NQ == 1 ? 1 : GDIM) lie side by side in source 0 (the
// velocity block, or a pressure / a scalar alone), every further one is a column of its own (a scalar inside the block of
// its group).  A partial row is [vol, s1 (NQ), s2 (NQ (NQ + 1) / 2, upper triangle row by row)].
__host__ __device__ constexpr int ox_prof_nr(int nq) { return 1 + nq + nq * (nq + 1) / 2; }

struct ProfSrc {
  const double *p[3];
  int64_t ld[3];
};

// the mean of basis function i over the cell: the row sum of the mean mass matrix (sum_j phi_j = 1)
template <int GDIM, int DEG>
__host__ __device__ constexpr double prof_mrow(int i) {
  double s = 0.0;
  for (int j = 0; j < ox_nd(GDIM, DEG); ++j) s += Diag<GDIM, DEG>::mass(i, j);
  return s;
}

// One 256-lane block per chunk (chunk[c] = {first entry of order, cells, bin, 1 if the cells are consecutive}), one lane
// per cell e = order[first + lane]; with delta_i = q_i - shift[bin] at the cell's nodes
//   s1[k] = |c| sum_i m_i delta_i[k],   s2[k][l] = |c| sum_i delta_i[k] (M delta[:, l])_i,  k <= l,
// summed over the chunk by the fixed tree of ox_block_sum_256 into partials[c].
template <int GDIM, int DEG, int NQ>
__global__ __launch_bounds__(256) void k_profile_cells(ox_cells cells, const int32_t *__restrict__ cell_dofs, ProfSrc src,
                                                       const int32_t *__restrict__ order, const int4 *__restrict__ chunk,
                                                       const double *__restrict__ shift, double *__restrict__ partials) {
  using E = Diag<GDIM, DEG>;
  constexpr int ND = ox_nd(GDIM, DEG), NR = ox_prof_nr(NQ), NC0 = NQ == 1 ? 1 : GDIM;
  __shared__ double lds[4 * NR];
  const int4 ch = chunk[blockIdx.x];
  const int len = ch.y < 256 ? ch.y : 256;
  double v[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = 0.0;
  int64_t e = -1;
  if ((int)threadIdx.x < len) e = ch.w ? (int64_t)order[ch.x] + threadIdx.x : (int64_t)order[(int64_t)ch.x + threadIdx.x];
  if (e >= 0 && e < cells.n_cells) {
    int32_t dd[ND];
    ox_load_dofs<ND>(cell_dofs, e, dd);
    const double adet = ox_geom_adet<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM));
    double q[ND][NQ];
    if (src.ld[0] == NC0) {
      double q0[ND][NC0];
      ox_gather<ND, NC0>(dd, src.p[0], q0);
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int c = 0; c < NC0; ++c) q[i][c] = q0[i][c];
    } else {
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int c = 0; c < NC0; ++c) q[i][c] = src.p[0][(size_t)dd[i] * src.ld[0] + c];
    }
#pragma unroll
    for (int k = NC0; k < NQ; ++k)
#pragma unroll
      for (int i = 0; i < ND; ++i) q[i][k] = src.p[1 + k - NC0][(size_t)dd[i] * src.ld[1 + k - NC0]];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const double sh = shift ? shift[(size_t)ch.z * NQ + k] : 0.0;
#pragma unroll
      for (int i = 0; i < ND; ++i) q[i][k] -= sh;
    }
    const double vol = ox_cell_volume<GDIM>(adet);
    v[0] = vol;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < ND; ++i)
        if (prof_mrow<GDIM, DEG>(i) != 0.0) s = fma(prof_mrow<GDIM, DEG>(i), q[i][k], s);
      v[1 + k] = vol * s;
    }
    double s2[NR - 1 - NQ];
#pragma unroll
    for (int m = 0; m < NR - 1 - NQ; ++m) s2[m] = 0.0;
#pragma unroll
    for (int l = 0; l < NQ; ++l)
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < ND; ++j)
          if (E::mass(i, j) != 0.0) r = fma(E::mass(i, j), q[j][l], r);
#pragma unroll
        for (int k = 0; k <= l; ++k) {  // (k, l), k <= l, sits at k NQ - k (k - 1) / 2 + l - k of the upper triangle
          const int m = k * NQ - k * (k - 1) / 2 + l - k;
          s2[m] = fma(q[i][k], r, s2[m]);
        }
      }
#pragma unroll
    for (int m = 0; m < NR - 1 - NQ; ++m) v[1 + NQ + m] = vol * s2[m];
  }
  ox_block_sum_256<NR>(v, lds);
  if (threadIdx.x == 0) {
    double *__restrict__ p = partials + (size_t)blockIdx.x * NR;
#pragma unroll
    for (int i = 0; i < NR; ++i) p[i] = v[i];
  }
}

// One wave per bin: the bin's chunk rows lane-strided in ascending order, a wave sum, and in lane 0 the weighted merge
// (a = w / (W + w), b = W a;  d = S1 / V, g = shift + d):
//   mean' = mean + a (g - mean),   M2' = M2 + w (S2 / V - d d^T) + b (g - mean) (g - mean)^T.
// seed: mean := S1 / V alone (the sums of a run with shift 0).  shift may BE mean (read before it is written).
template <int NQ>
__global__ __launch_bounds__(64) void k_profile_update(const int32_t *__restrict__ bin_chunk_ptr,
                                                       const double *__restrict__ partials, const double *shift, double w,
                                                       double a, double b, int seed, double *mean, double *__restrict__ m2,
                                                       double *__restrict__ vol, double *__restrict__ sums) {
  constexpr int NR = ox_prof_nr(NQ), NV = NQ * (NQ + 1) / 2;
  const int64_t bin = blockIdx.x;
  const int c0 = bin_chunk_ptr[bin], c1 = bin_chunk_ptr[bin + 1];
  double v[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = 0.0;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) {
    const double *__restrict__ p = partials + (size_t)c * NR;
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] += p[i];
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) v[i] = ox_wave_sum(v[i]);
  if (threadIdx.x != 0) return;
  if (sums) {
#pragma unroll
    for (int i = 0; i < NR; ++i) sums[(size_t)bin * NR + i] = v[i];
  }
  vol[bin] = v[0];
  const double inv = 1.0 / v[0];
  double d[NQ], dl[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) d[k] = v[1 + k] * inv;
  if (seed) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) mean[(size_t)bin * NQ + k] = d[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const double mk = mean[(size_t)bin * NQ + k];
    const double g = (shift ? shift[(size_t)bin * NQ + k] : 0.0) + d[k];
    dl[k] = g - mk;
    mean[(size_t)bin * NQ + k] = fma(a, dl[k], mk);
  }
  int m = 0;
#pragma unroll
  for (int k = 0; k < NQ; ++k)
#pragma unroll
    for (int l = k; l < NQ; ++l, ++m) {
      const double c = fma(-d[k], d[l], v[1 + NQ + m] * inv);
      m2[(size_t)bin * NV + m] = fma(b * dl[k], dl[l], fma(w, c, m2[(size_t)bin * NV + m]));
    }
}

}  // namespace

extern "C" int ox_profile_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, int nq, int n_src,
                                const double *const *src, const int64_t *ld, const int32_t *order, const int32_t *chunks,
                                int64_t n_chunks, const double *shift, double *partials, void *stream) {
  if (!cells || !cell_dofs || !src || !ld || !order || !chunks || !partials || !cells->geom)
    OX_FAIL("ox_profile_cells: null argument");
  if (cells->n_cells <= 0 || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_profile_cells: %lld cells", (long long)cells->n_cells);
  if (n_chunks <= 0 || n_chunks > (int64_t)0x7fffffff) OX_FAIL("ox_profile_cells: n_chunks=%lld", (long long)n_chunks);
  const int g = cells->gdim;
  if (!(nq == 1 || (nq >= g && nq <= g + 2))) OX_FAIL("ox_profile_cells: nq=%d on gdim=%d (1 or gdim .. gdim + 2)", nq, g);
  const int nc0 = nq == 1 ? 1 : g;
  if (n_src != 1 + nq - nc0) OX_FAIL("ox_profile_cells: nq=%d takes %d sources, not %d", nq, 1 + nq - nc0, n_src);
  ProfSrc s{};
  for (int i = 0; i < n_src; ++i) {
    if (!src[i] || ld[i] < (i == 0 ? nc0 : 1)) OX_FAIL("ox_profile_cells: source %d: null or ld=%lld", i, (long long)ld[i]);
    s.p[i] = src[i], s.ld[i] = ld[i];
  }
  hipStream_t st = ox_stream(stream);
  const int4 *ch = reinterpret_cast<const int4 *>(chunks);
#define OX_PROF_LAUNCH(GD, DG, NQ_)                                                                                     \
  if (nq == NQ_) {                                                                                                      \
    hipLaunchKernelGGL((k_profile_cells<GD, DG, NQ_>), dim3((unsigned)n_chunks), dim3(256), 0, st, *cells, cell_dofs, s, \
                       order, ch, shift, partials);                                                                     \
  }
#define OX_PROF_CASE(GD, DG)                                                                                    \
  if (g == GD && degree == DG) {                                                                                \
    if (ox_prof_on) ox_prof_start(OX_TAG_PROFILE_CELLS, st, n_chunks);                                          \
    OX_PROF_LAUNCH(GD, DG, 1)                                                                                   \
    OX_PROF_LAUNCH(GD, DG, GD) OX_PROF_LAUNCH(GD, DG, GD + 1) OX_PROF_LAUNCH(GD, DG, GD + 2)                    \
    if (ox_prof_on) ox_prof_stop(st);                                                                           \
    OX_LAUNCH_CHECK();                                                                                          \
    return 0;                                                                                                   \
  }
  OX_FOR_GDIM_DEG(OX_PROF_CASE)
#undef OX_PROF_CASE
#undef OX_PROF_LAUNCH
  OX_FAIL("ox_profile_cells: unsupported gdim=%d degree=%d", g, degree);
}

extern "C" int ox_profile_update(int nq, int64_t n_bins, const int32_t *bin_chunk_ptr, const double *partials,
                                 const double *shift, double w, double W_old, int seed, double *mean, double *m2, double *vol,
                                 double *sums, void *stream) {
  if (!bin_chunk_ptr || !partials || !mean || !vol || (!seed && !m2)) OX_FAIL("ox_profile_update: null argument");
  if (nq < 1 || nq > 5) OX_FAIL("ox_profile_update: nq=%d", nq);
  if (n_bins <= 0 || n_bins > (int64_t)0x7fffffff) OX_FAIL("ox_profile_update: n_bins=%lld", (long long)n_bins);
  double a = 0.0, b = 0.0;
  if (!seed) {
    if (!(w > 0.0) || !std::isfinite(w)) OX_FAIL("ox_profile_update: w=%g", w);
    if (!(W_old >= 0.0) || !std::isfinite(W_old)) OX_FAIL("ox_profile_update: W_old=%g", W_old);
    a = w / (W_old + w), b = W_old * a;
  }
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_PROFILE_UPDATE, st, n_bins);
#define OX_PROF_UPD(NQ_)                                                                                                  \
  if (nq == NQ_)                                                                                                          \
    hipLaunchKernelGGL((k_profile_update<NQ_>), dim3((unsigned)n_bins), dim3(64), 0, st, bin_chunk_ptr, partials, shift, w, \
                       a, b, seed, mean, m2, vol, sums);
  OX_PROF_UPD(1) OX_PROF_UPD(2) OX_PROF_UPD(3) OX_PROF_UPD(4) OX_PROF_UPD(5)
#undef OX_PROF_UPD
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_flow_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *u, const double *nut,
                             double dt, double nu, double *fields, double *cell_integrals, double *partials, void *stream) {
  if (!cells || !cell_dofs || !u || !partials || !cells->geom) OX_FAIL("ox_flow_cells: null argument");
  if (!(dt > 0.0) || !std::isfinite(dt)) OX_FAIL("ox_flow_cells: dt=%g", dt);
  if (!(nu >= 0.0) || !std::isfinite(nu)) OX_FAIL("ox_flow_cells: nu=%g", nu);
  if (cells->n_cells <= 0) OX_FAIL("ox_flow_cells: %lld cells", (long long)cells->n_cells);
  const int64_t nblk = ox_cell_blocks("ox_flow_cells", cells);
  if (nblk < 0) return -1;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
#define OX_FLOW_CASE(GD, DG)                                                                                              \
  if (g == GD && degree == DG) {                                                                                          \
    if (ox_prof_on) ox_prof_start(OX_TAG_FLOW_CELLS, st, cells->n_cells);                                                 \
    hipLaunchKernelGGL((k_flow_cells<GD, DG>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, u, nut, dt, nu, fields,   \
                       cell_integrals, partials);                                                                         \
    if (ox_prof_on) ox_prof_stop(st);                                                                                     \
    OX_LAUNCH_CHECK();                                                                                                    \
    return 0;                                                                                                             \
  }
  OX_FOR_GDIM_DEG(OX_FLOW_CASE)
#undef OX_FLOW_CASE
  OX_FAIL("ox_flow_cells: unsupported gdim=%d degree=%d", g, degree);
}

extern "C" int ox_flow_reduce(int64_t n_blocks, const double *partials, double *ring, int64_t capacity, int64_t slot,
                              void *stream) {
  if (!partials || !ring) OX_FAIL("ox_flow_reduce: null argument");
  if (n_blocks <= 0) OX_FAIL("ox_flow_reduce: n_blocks=%lld", (long long)n_blocks);
  if (slot < 0 || slot >= capacity) OX_FAIL("ox_flow_reduce: slot %lld of %lld", (long long)slot, (long long)capacity);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_FLOW_REDUCE, st, n_blocks);
  hipLaunchKernelGGL(k_flow_reduce, dim3(1), dim3(256), 0, st, n_blocks, partials, ring + (size_t)slot * 8);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_stats_accumulate(int ncomp, int64_t n, const double *x, int64_t ldx, double w, double W_old, double *mean,
                                   double *cov, void *stream) {
  if (!x || !mean || !cov) OX_FAIL("ox_stats_accumulate: null argument");
  if (ncomp < 1 || ncomp > 3) OX_FAIL("ox_stats_accumulate: ncomp=%d", ncomp);
  if (!(w > 0.0) || !std::isfinite(w)) OX_FAIL("ox_stats_accumulate: w=%g", w);
  if (!(W_old >= 0.0) || !std::isfinite(W_old)) OX_FAIL("ox_stats_accumulate: W_old=%g", W_old);
  if (ldx < ncomp) OX_FAIL("ox_stats_accumulate: ldx=%lld < ncomp=%d", (long long)ldx, ncomp);
  if (n <= 0) return 0;
  if (n > (int64_t)0x7fffffff * 128) OX_FAIL("ox_stats_accumulate: n=%lld", (long long)n);
  hipStream_t st = ox_stream(stream);
  const double Wn = W_old + w;
  const double a = w / Wn, b = W_old * a;
  const int first = W_old == 0.0;
  const bool vec = ldx == ncomp && (((uintptr_t)x | (uintptr_t)mean | (uintptr_t)cov) & 15) == 0;
  const int64_t threads = (ncomp == 1 && vec) ? n / 2 + 1 : n;
  const unsigned nblk = (unsigned)((threads + 255) / 256);
  if (ox_prof_on) ox_prof_start(OX_TAG_STATS_ACCUMULATE, st, n * ncomp);
#define OX_STATS_CASE(NC)                                                                                              \
  if (ncomp == NC) {                                                                                                   \
    if (vec) hipLaunchKernelGGL((k_stats<NC, true>), dim3(nblk), dim3(256), 0, st, n, x, ldx, a, b, first, mean, cov); \
    else hipLaunchKernelGGL((k_stats<NC, false>), dim3(nblk), dim3(256), 0, st, n, x, ldx, a, b, first, mean, cov);    \
  }
  OX_STATS_CASE(1) OX_STATS_CASE(2) OX_STATS_CASE(3)
#undef OX_STATS_CASE
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}
