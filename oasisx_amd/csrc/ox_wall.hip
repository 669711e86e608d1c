// Wall shear stress, traction and boundary forces on tagged exterior facets.
//
// Facet f of cell c, opposite local vertex a; G_b = grad lambda_b of the cell (G_0 = -sum_b G_b), |det J| from the
// cell's geometry record:
//   n     = -G_a / |G_a|                         outward unit normal
//   |f|   = |det J| |G_a| / (gdim - 1)!
//   gbar[d][k] = sum_i u[dof_i][d] sum_b mean_f(dphi_i/dlambda_b) G[b][k]      facet mean of grad u
//   pbar  = sum_j p[dof_j] mean_f(psi_j)                                        facet mean of p
//   t     = -pbar n + nu_eff (gbar + gbar^T) n,   nu_eff = nu + nut[c] (nut may be NULL)
//   wss   = t - (t.n) n
//
// k_wall_stress: one lane per facet.  Streamed per facet: the record (kernel cell index, local facet; 8 B), and through
// LDS, so that a block writes whole contiguous rows, t, wss and |f| t (and, with weight > 0, the read-modify-write of the
// accumulators).  Gathered: the cell's two dof lists and geometry record, the ND x GDIM velocity and NDQ pressure values.
// The facet means of the basis are compile-time constants (fe_tables_f.h): identically-zero entries cost nothing; the
// local facet selects one of GDIM + 1 instantiations of the contraction.  No atomics; every sum has a fixed order.
// k_wall_forces: one block per tag sums its contiguous segment of |f| t (lane-strided partial sums in ascending facet
// order, then the fixed tree of ox_block_sum_256) and writes -rho sum into slot k of a ring (capacity, n_tags, gdim).
#include "ox_element.h"

namespace {

#define OX_WALL_NS 5  // rows staged per block: t, wss, |f| t, weight wss, weight t

template <int GDIM, int DU, int DP>
__global__ __launch_bounds__(256) void k_wall_stress(ox_cells cells, const int32_t *__restrict__ vdofs,
                                                     const int32_t *__restrict__ qdofs, int64_t n_facets,
                                                     const int2 *__restrict__ rec, const double *__restrict__ u,
                                                     const double *__restrict__ p, const double *__restrict__ nut,
                                                     double nu, double weight, double *__restrict__ out_t,
                                                     double *__restrict__ out_wss, double *__restrict__ out_ft,
                                                     double *__restrict__ acc_vec, double *__restrict__ acc_mag,
                                                     double *__restrict__ acc_t) {
  constexpr int ND = ox_nd(GDIM, DU), NDQ = ox_nd(GDIM, DP);
  __shared__ double lds[OX_WALL_NS][256 * GDIM];
  const int64_t f0 = (int64_t)blockIdx.x * 256;
  const int64_t f = f0 + threadIdx.x;
  const bool acc = weight > 0.0;
  double t[GDIM], wss[GDIM], ft[GDIM];
  double mag = 0.0;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int d = 0; d < GDIM; ++d) t[d] = wss[d] = ft[d] = qnan;
  bool live = f < n_facets;
  if (live) {
    const int2 r = rec[f];
    // a record outside the tables reads nothing and leaves NaN in the facet's rows
    live = r.x >= 0 && (int64_t)r.x < cells.n_cells && r.y >= 0 && r.y <= GDIM;
    if (live) {
      const int64_t e = r.x;
      const int a = r.y;
      int32_t dv[ND], dq[NDQ];
      ox_load_dofs<ND>(vdofs, e, dv);
      ox_load_dofs<NDQ>(qdofs, e, dq);
      double G[GDIM + 1][GDIM], adet;
      ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
      const double nu_eff = nut ? nu + nut[e] : nu;
      double uc[ND][GDIM], pc[NDQ][1];
      ox_gather<ND, GDIM>(dv, u, uc);
      ox_gather<NDQ, 1>(dq, p, pc);
      // tb[d][b] = sum_i u_i[d] mean_f(dphi_i/dlambda_b) and pbar = sum_j p_j mean_f(psi_j) on the local facet, in dof
      // order; Ga = grad lambda_a
      double tb[GDIM][GDIM + 1] = {}, pbar = 0.0, Ga[GDIM] = {};
      ox_facet_dispatch<GDIM>(a, [&](auto facet) {
        constexpr int A = decltype(facet)::value;
        ox_contract<GDIM, ND>(uc, ox_dphif<GDIM, DU>()[A], tb);
#pragma unroll
        for (int j = 0; j < NDQ; ++j)
          if (ox_phif<GDIM, DP>()[A][j] != 0.0) pbar = fma(pc[j][0], ox_phif<GDIM, DP>()[A][j], pbar);
#pragma unroll
        for (int d = 0; d < GDIM; ++d) Ga[d] = G[A][d];
      });
      double g[GDIM][GDIM], n[GDIM], area;
      ox_grad_from_t<GDIM>(tb, G, g);
      ox_facet_normal<GDIM>(Ga, adet, n, area);
      double tn = 0.0;
#pragma unroll
      for (int d = 0; d < GDIM; ++d) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < GDIM; ++k) s = fma(g[d][k] + g[k][d], n[k], s);
        t[d] = fma(nu_eff, s, -pbar * n[d]);
        tn = fma(t[d], n[d], tn);
      }
#pragma unroll
      for (int d = 0; d < GDIM; ++d) {
        wss[d] = fma(-tn, n[d], t[d]);
        ft[d] = area * t[d];
      }
      // |wss|: squares and sums rounded one by one (the statistics are the same sums as a host evaluation of them)
      double m2 = __dmul_rn(wss[0], wss[0]);
#pragma unroll
      for (int d = 1; d < GDIM; ++d) m2 = __dadd_rn(m2, __dmul_rn(wss[d], wss[d]));
      mag = sqrt(m2);
    }
  }
  // rows of this block through LDS: lane l holds facet f0 + l, the block writes [f0 * GDIM, (f0 + 256) * GDIM)
#pragma unroll
  for (int d = 0; d < GDIM; ++d) {
    lds[0][threadIdx.x * GDIM + d] = t[d];
    lds[1][threadIdx.x * GDIM + d] = wss[d];
    lds[2][threadIdx.x * GDIM + d] = ft[d];
    if (acc) {
      lds[3][threadIdx.x * GDIM + d] = __dmul_rn(weight, wss[d]);
      lds[4][threadIdx.x * GDIM + d] = __dmul_rn(weight, t[d]);
    }
  }
  __syncthreads();
  const int64_t nrem = n_facets - f0;
  const int nval = (int)(nrem < 256 ? nrem : 256) * GDIM;
  const size_t base = (size_t)f0 * GDIM;
#pragma unroll
  for (int k = 0; k < GDIM; ++k) {
    const int j = threadIdx.x + k * 256;
    if (j < nval) {
      out_t[base + j] = lds[0][j];
      out_wss[base + j] = lds[1][j];
      out_ft[base + j] = lds[2][j];
      if (acc) {
        acc_vec[base + j] = __dadd_rn(acc_vec[base + j], lds[3][j]);
        acc_t[base + j] = __dadd_rn(acc_t[base + j], lds[4][j]);
      }
    }
  }
  if (acc && f < n_facets) acc_mag[f] = __dadd_rn(acc_mag[f], __dmul_rn(weight, mag));
}

template <int GDIM>
__global__ __launch_bounds__(256) void k_wall_forces(const int64_t *__restrict__ tag_ptr, const double *__restrict__ ft,
                                                     double mrho, double *__restrict__ ring, int n_tags, int64_t slot) {
  __shared__ double lds[4 * GDIM];
  const int tag = blockIdx.x;
  const int64_t f0 = tag_ptr[tag], f1 = tag_ptr[tag + 1];
  double v[GDIM];
#pragma unroll
  for (int d = 0; d < GDIM; ++d) v[d] = 0.0;
#pragma unroll 4
  for (int64_t f = f0 + threadIdx.x; f < f1; f += 256)
#pragma unroll
    for (int d = 0; d < GDIM; ++d) v[d] += ft[(size_t)f * GDIM + d];
  ox_block_sum_256<GDIM>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int d = 0; d < GDIM; ++d) ring[((size_t)slot * n_tags + tag) * GDIM + d] = mrho * v[d];
  }
}

}  // namespace

extern "C" int ox_wall_stress(int u_degree, int p_degree, const ox_cells *cells, const int32_t *cell_vdofs,
                              const int32_t *cell_qdofs, int64_t n_facets, const int32_t *facet_rec, const double *u,
                              const double *p, const double *nut, double nu, double weight, double *t, double *wss,
                              double *ft, double *acc_vec, double *acc_mag, double *acc_t, void *stream) {
  if (!cells || !cells->geom || !cell_vdofs || !cell_qdofs || !facet_rec || !u || !p || !t || !wss || !ft)
    OX_FAIL("ox_wall_stress: null argument");
  if (weight > 0.0 && (!acc_vec || !acc_mag || !acc_t)) OX_FAIL("ox_wall_stress: weight > 0 without accumulators");
  if (!(weight >= 0.0)) OX_FAIL("ox_wall_stress: weight=%g", weight);
  if (n_facets <= 0) return 0;
  if (n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_wall_stress: %lld facets, %lld cells", (long long)n_facets, (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_facets + 255) / 256);
  // P1-P1, P2-P1, P3-P2: the pressure degree follows from the velocity's
#define OX_WALL_CASE(GD, DU)                                                                                            \
  if (g == GD && u_degree == DU && p_degree == (DU == 3 ? 2 : 1)) {                                                     \
    if (ox_prof_on) ox_prof_start(OX_TAG_WALL_STRESS, st, n_facets);                                                    \
    hipLaunchKernelGGL((k_wall_stress<GD, DU, (DU == 3 ? 2 : 1)>), dim3(nblk), dim3(256), 0, st, *cells, cell_vdofs,    \
                       cell_qdofs, n_facets, reinterpret_cast<const int2 *>(facet_rec), u, p, nut, nu, weight, t, wss,  \
                       ft, acc_vec, acc_mag, acc_t);                                                                    \
    if (ox_prof_on) ox_prof_stop(st);                                                                                   \
    OX_LAUNCH_CHECK();                                                                                                  \
    return 0;                                                                                                           \
  }
  OX_FOR_GDIM_DEG(OX_WALL_CASE)
#undef OX_WALL_CASE
  OX_FAIL("ox_wall_stress: unsupported gdim=%d, P%d-P%d", g, u_degree, p_degree);
}

extern "C" int ox_wall_forces(int gdim, int n_tags, const int64_t *tag_ptr, const double *ft, double rho, double *ring,
                              int64_t capacity, int64_t slot, void *stream) {
  if (!tag_ptr || !ft || !ring) OX_FAIL("ox_wall_forces: null argument");
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_wall_forces: gdim=%d", gdim);
  if (n_tags <= 0) OX_FAIL("ox_wall_forces: n_tags=%d", n_tags);
  if (slot < 0 || slot >= capacity) OX_FAIL("ox_wall_forces: slot %lld of %lld", (long long)slot, (long long)capacity);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_WALL_FORCES, st, n_tags);
  if (gdim == 2) hipLaunchKernelGGL((k_wall_forces<2>), dim3(n_tags), dim3(256), 0, st, tag_ptr, ft, -rho, ring, n_tags, slot);
  else hipLaunchKernelGGL((k_wall_forces<3>), dim3(n_tags), dim3(256), 0, st, tag_ptr, ft, -rho, ring, n_tags, slot);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}
