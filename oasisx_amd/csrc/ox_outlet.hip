// Outlet models on tagged exterior facets: flow rates, lumped resistance / RCR Windkessel pressures and the backflow
// stabilisation of a pressure boundary.
//
// Facet f of cell c, opposite local vertex a, as in ox_wall.hip: n = -G_a / |G_a| (outward), |f| = |det J| |G_a| / (gdim-1)!.
//   flux_f = |f| n . ubar_f,  ubar_f = sum_i u[dof_i] mean_f(phi_i)          the facet mean is exact (compile-time tables)
//   Q_tag  = sum_{f in tag} flux_f                                            Q > 0 leaves the domain
//   model of a tag (explicit in Q):  C dPc/dt = Q - (Pc - p_distal)/Rd by backward Euler,  P = Pc + Rp Q,  h = P / rho
//   backflow:  A[r][s] += (beta_f/2) |f| sum_q w_q max(-u_ab(x_q).n, 0) phi_r(x_q) phi_s(x_q),  b_first[r] -= (same) u1[s]
//
// k_outlet_flux: one lane per facet; streamed: the record (8 B) and the result (8 B); gathered: the dofs of the cell that
// live on the facet with a nonzero mean, their velocities, the geometry record.  The local facet selects one of GDIM + 1
// instantiations of the contraction, whose identically-zero entries cost nothing.
// k_outlet_update: one block per tag; lane-strided partial sums in ascending facet order, then the fixed tree of
// ox_block_sum_256; thread 0 writes Q, advances the tag's model and writes (Q, P, Pc); after a barrier all lanes write h on
// the tag's pressure dofs.
// k_outlet_backflow: one lane per touched velocity row; the row's (facet, position of the row among the facet's dofs)
// pairs in ascending facet id, the slots of A's value array from set-up.  The lane owns its row of A and of b_first: no
// atomics, a fixed order of sums.
#include "ox_element.h"

namespace {

template <int GDIM, int DU>
__global__ __launch_bounds__(256) void k_outlet_flux(ox_cells cells, const int32_t *__restrict__ vdofs, int64_t n_facets,
                                                     const int2 *__restrict__ rec, const double *__restrict__ u,
                                                     double *__restrict__ flux) {
  constexpr int ND = ox_nd(GDIM, DU);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_facets) return;
  const int2 r = rec[f];
  // a record outside the tables reads nothing and leaves NaN
  if (!(r.x >= 0 && (int64_t)r.x < cells.n_cells && r.y >= 0 && r.y <= GDIM)) {
    flux[f] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  const int64_t e = r.x;
  const int32_t *__restrict__ dv = vdofs + (size_t)e * ND;
  double n[GDIM], area, ub[GDIM] = {};
  ox_facet_geometry<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), r.y, n, area);
  // ub[d] = sum_i u[dof_i][d] mean_f(phi_i) on the local facet, in dof order; dofs with a zero mean are not read
  ox_facet_dispatch<GDIM>(r.y, [&](auto facet) {
    constexpr int A = decltype(facet)::value;
#pragma unroll
    for (int i = 0; i < ND; ++i)
      if (ox_phif<GDIM, DU>()[A][i] != 0.0) {
        const size_t dof = (size_t)dv[i];
#pragma unroll
        for (int d = 0; d < GDIM; ++d) ub[d] = fma(u[dof * GDIM + d], ox_phif<GDIM, DU>()[A][i], ub[d]);
      }
  });
  double q = 0.0;
#pragma unroll
  for (int d = 0; d < GDIM; ++d) q = fma(n[d], ub[d], q);
  flux[f] = area * q;
}

#define OX_OUTLET_NPAR 8  // per tag: kind (0 none, 1 resistance, 2 RCR), Rp, C, Rd, p_distal, rho, 2 reserved

__global__ __launch_bounds__(256) void k_outlet_update(const int64_t *__restrict__ tag_ptr, const double *__restrict__ flux,
                                                       double *__restrict__ ring, int n_tags, int64_t slot,
                                                       const double *__restrict__ params, double dt,
                                                       double *__restrict__ state, double *__restrict__ hist,
                                                       const int64_t *__restrict__ dof_ptr, const int32_t *__restrict__ dofs,
                                                       double *__restrict__ h, int64_t h_stride) {
  __shared__ double lds[4];
  __shared__ double hval;
  const int tag = blockIdx.x;
  const int64_t f0 = tag_ptr[tag], f1 = tag_ptr[tag + 1];
  double v[1] = {0.0};
#pragma unroll 4
  for (int64_t f = f0 + threadIdx.x; f < f1; f += 256) v[0] += flux[f];
  ox_block_sum_256<1>(v, lds);
  const int kind = params ? (int)params[(size_t)tag * OX_OUTLET_NPAR] : 0;  // the same in every lane of the block
  if (threadIdx.x == 0) {
    const double Q = v[0];
    ring[(size_t)slot * n_tags + tag] = Q;
    if (kind != 0) {
      const double *__restrict__ p = params + (size_t)tag * OX_OUTLET_NPAR;
      const double Rp = p[1], C = p[2], Rd = p[3], pd = p[4], rho = p[5];
      double Pc = state[tag];
      if (kind == 2) {
        // backward Euler; Rd = 0 is the limit Pc = p_distal
        Pc = Rd > 0.0 ? (Pc + (dt / C) * (Q + pd / Rd)) / (1.0 + dt / (Rd * C)) : pd;
        state[tag] = Pc;
      }
      const double P = Pc + Rp * Q;
      double *__restrict__ hs = hist + ((size_t)slot * n_tags + tag) * 3;
      hs[0] = Q;
      hs[1] = P;
      hs[2] = Pc;
      hval = P / rho;
    }
  }
  if (kind == 0) return;
  __syncthreads();
  const double hv = hval;
  double *__restrict__ ht = h + (size_t)tag * h_stride;
  for (int64_t j = dof_ptr[tag] + threadIdx.x; j < dof_ptr[tag + 1]; j += 256) {
    const int64_t dof = dofs[j];
    if (dof >= 0 && dof < h_stride) ht[dof] = hv;
  }
}

template <int GDIM, int DU>
__global__ __launch_bounds__(256) void k_outlet_backflow(ox_cells cells, const int32_t *__restrict__ vdofs, int64_t n_rows,
                                                         const int32_t *__restrict__ rows, const int64_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ pair_facet,
                                                         const int32_t *__restrict__ pair_loc,
                                                         const int64_t *__restrict__ pair_off, int64_t n_facets,
                                                         const int2 *__restrict__ rec, const double *__restrict__ beta,
                                                         const double *__restrict__ uab, const double *__restrict__ u1,
                                                         double *__restrict__ avals, int64_t a_size,
                                                         double *__restrict__ b_first) {
  using O = ox_facet_rule<GDIM, DU>;
  constexpr int ND = ox_nd(GDIM, DU), NFD = O::NFD;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  double acc[GDIM];
#pragma unroll
  for (int d = 0; d < GDIM; ++d) acc[d] = 0.0;
  for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
    const int64_t fi = pair_facet[k];
    const int jr = pair_loc[k];
    if (fi < 0 || fi >= n_facets || jr < 0 || jr >= NFD) continue;  // a pair outside the tables adds nothing
    const int2 r = rec[fi];
    if (!(r.x >= 0 && (int64_t)r.x < cells.n_cells && r.y >= 0 && r.y <= GDIM)) continue;
    const int64_t e = r.x;
    const int a = r.y;
    double n[GDIM], area;
    ox_facet_geometry<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), a, n, area);
    const double c = 0.5 * beta[fi] * area;
    size_t dvf[NFD];
    double un[NFD], ent[NFD];
#pragma unroll
    for (int j = 0; j < NFD; ++j) {
      dvf[j] = (size_t)vdofs[(size_t)e * ND + O::fd(a, j)];
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < GDIM; ++d) s = fma(uab[dvf[j] * GDIM + d], n[d], s);
      un[j] = s;
      ent[j] = 0.0;
    }
    for (int q = 0; q < O::NQ; ++q) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NFD; ++j) s = fma(O::phi(q, j), un[j], s);
      const double gr = O::w(q) * fmax(-s, 0.0) * O::phi(q, jr);
#pragma unroll
      for (int j = 0; j < NFD; ++j) ent[j] = fma(gr, O::phi(q, j), ent[j]);
    }
#pragma unroll
    for (int j = 0; j < NFD; ++j) {
      const double v = c * ent[j];
      const int64_t off = pair_off[(size_t)k * NFD + j];
      if (off >= 0 && off < a_size) avals[off] += v;
#pragma unroll
      for (int d = 0; d < GDIM; ++d) acc[d] = fma(-v, u1[dvf[j] * GDIM + d], acc[d]);
    }
  }
  const size_t row = (size_t)rows[i];
#pragma unroll
  for (int d = 0; d < GDIM; ++d) b_first[row * GDIM + d] += acc[d];
}

}  // namespace

extern "C" int ox_outlet_flux(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_facets,
                              const int32_t *facet_rec, const double *u, double *flux, void *stream) {
  if (!cells || !cells->geom || !cell_vdofs || !facet_rec || !u || !flux) OX_FAIL("ox_outlet_flux: null argument");
  if (n_facets <= 0) return 0;
  if (n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_outlet_flux: %lld facets, %lld cells", (long long)n_facets, (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_facets + 255) / 256);
#define OX_OUTLET_FLUX_CASE(GD, DU)                                                                                \
  if (g == GD && u_degree == DU) {                                                                                 \
    if (ox_prof_on) ox_prof_start(OX_TAG_OUTLET_FLUX, st, n_facets);                                               \
    hipLaunchKernelGGL((k_outlet_flux<GD, DU>), dim3(nblk), dim3(256), 0, st, *cells, cell_vdofs, n_facets,        \
                       reinterpret_cast<const int2 *>(facet_rec), u, flux);                                        \
    if (ox_prof_on) ox_prof_stop(st);                                                                              \
    OX_LAUNCH_CHECK();                                                                                             \
    return 0;                                                                                                      \
  }
  OX_FOR_GDIM_DEG(OX_OUTLET_FLUX_CASE)
#undef OX_OUTLET_FLUX_CASE
  OX_FAIL("ox_outlet_flux: unsupported gdim=%d, P%d", g, u_degree);
}

extern "C" int ox_outlet_update(int n_tags, const int64_t *tag_ptr, const double *flux, double *ring, int64_t capacity,
                                int64_t slot, const double *params, double dt, double *state, double *hist,
                                const int64_t *dof_ptr, const int32_t *dofs, double *h, int64_t h_stride, void *stream) {
  if (!tag_ptr || !flux || !ring) OX_FAIL("ox_outlet_update: null argument");
  if (n_tags <= 0) OX_FAIL("ox_outlet_update: n_tags=%d", n_tags);
  if (slot < 0 || slot >= capacity) OX_FAIL("ox_outlet_update: slot %lld of %lld", (long long)slot, (long long)capacity);
  if (params) {
    if (!state || !hist || !dof_ptr || !dofs || !h || h_stride <= 0) OX_FAIL("ox_outlet_update: models without their arrays");
    if (!(dt > 0.0)) OX_FAIL("ox_outlet_update: dt=%g", dt);
  }
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_OUTLET_UPDATE, st, n_tags);
  hipLaunchKernelGGL(k_outlet_update, dim3(n_tags), dim3(256), 0, st, tag_ptr, flux, ring, n_tags, slot, params, dt, state,
                     hist, dof_ptr, dofs, h, h_stride);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_outlet_backflow(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_rows,
                                  const int32_t *rows, const int64_t *row_ptr, const int32_t *pair_facet,
                                  const int32_t *pair_loc, const int64_t *pair_off, int64_t n_facets,
                                  const int32_t *facet_rec, const double *beta, const double *uab, const double *u1,
                                  double *a_vals, int64_t a_size, double *b_first, void *stream) {
  if (!cells || !cells->geom || !cell_vdofs || !rows || !row_ptr || !pair_facet || !pair_loc || !pair_off || !facet_rec ||
      !beta || !uab || !u1 || !a_vals || !b_first)
    OX_FAIL("ox_outlet_backflow: null argument");
  if (n_rows <= 0) return 0;
  if (n_rows > (int64_t)0x7fffffff || n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_outlet_backflow: %lld rows, %lld facets, %lld cells", (long long)n_rows, (long long)n_facets,
            (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_rows + 255) / 256);
#define OX_OUTLET_BACK_CASE(GD, DU)                                                                                   \
  if (g == GD && u_degree == DU) {                                                                                    \
    if (ox_prof_on) ox_prof_start(OX_TAG_OUTLET_BACKFLOW, st, n_rows);                                                \
    hipLaunchKernelGGL((k_outlet_backflow<GD, DU>), dim3(nblk), dim3(256), 0, st, *cells, cell_vdofs, n_rows, rows,   \
                       row_ptr, pair_facet, pair_loc, pair_off, n_facets, reinterpret_cast<const int2 *>(facet_rec),  \
                       beta, uab, u1, a_vals, a_size, b_first);                                                       \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_OUTLET_BACK_CASE)
#undef OX_OUTLET_BACK_CASE
  OX_FAIL("ox_outlet_backflow: unsupported gdim=%d, P%d", g, u_degree);
}
