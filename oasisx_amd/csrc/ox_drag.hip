// Drag zones: the volume term -sigma(x, |u|) (u - u_t) of porous media (Darcy-Forchheimer), sponge layers and solids by
// Brinkman penalisation.
//
// Cell e of a zone, M_e its mass matrix on the velocity component space, |e| = |det J| / gdim!:
//   sigma_e = alpha_e + beta_e |w(x_e)|,  w = u_ab - u_t at the centroid x_e          (k_drag_sigma)
//   D       = sum_e sigma_e M_e,   M_e[i][j] = |e| MASSD[i][j]  (the mean of phi_i phi_j, a compile-time table)
//   A += theta D,   b_first[r][:] += sum_(e, j) sigma_e M_e[i_r][j] w[dof_j][:],  w = u_t - (1 - theta) u_1     (k_drag_rows)
//   ft_e[:] = sigma_e int_e (u - u_t) dx = sigma_e |e| sum_j mean(phi_j) (u - u_t)[dof_j][:]            (k_drag_force_cells)
//
// k_drag_sigma: one lane per zone cell over the list of kernel cell positions; streamed: the list, alpha, beta (20 B) and
// the result; gathered: the cell's dofs and the velocities at them.
// k_drag_rows: one wave per touched slice, lane = row.  The lane walks its (cell, local index) pairs in the SELL order of
// the adjacency, skips the cells with sigma = 0, and sums the pair's nd entries at their in-row positions (the position
// bytes of the adjacency) into a wave-private accumulator in LDS whose columns are private to the lanes, and its share of
// the right-hand side in registers; the epilogue adds the accumulator to the row's entries of A once, 16 bytes per access
// (the slot arithmetic of the SELL storage).  Measured at 128^3 P2: adding every pair's entries straight to A in global
// memory, 10 scattered read-modify-writes per pair, took 11.9 ms for a whole-domain zone, this form 4.4.  The lane owns
// its row of the matrix and of the vector: no atomics, one order of sums, equal bits for equal inputs.
// k_drag_force_cells: one lane per zone cell; the sums per zone are ox_wall_forces' (one block per tag, a fixed tree).
#include "fe_tables_d.h"
#include "ox_element.h"

namespace {

template <int GDIM, int DEG>
struct Drag {
  static constexpr int ND = ox_nd(GDIM, DEG);
  static constexpr int PW = DEG == 1 ? 4 : (DEG == 2 ? (GDIM == 2 ? 8 : 16) : (GDIM == 2 ? 16 : 32));  // adj_pos stride
  __host__ __device__ static constexpr double phic(int i) { OX_FE_PICK(GDIM, DEG, OX_PHIC, [i]); }
  __host__ __device__ static constexpr double mass(int i, int j) { OX_FE_PICK(GDIM, DEG, OX_MASSD, [i][j]); }
  // mean of phi_j over the cell: the column sum of the mass table (sum_i phi_i = 1)
  __host__ __device__ static constexpr double colsum(int j) {
    double s = 0.0;
    for (int i = 0; i < ND; ++i) s += mass(i, j);
    return s;
  }
};

// w[i][d] = u[dof_i][d] - ut[dof_i][d] (ut == nullptr: u)
template <int GDIM, int ND>
__device__ __forceinline__ void drag_gather(const int32_t (&dd)[ND], const double *__restrict__ u,
                                            const double *__restrict__ ut, double (&w)[ND][GDIM]) {
  ox_gather<ND, GDIM>(dd, u, w);
  if (ut) {
    double t[ND][GDIM];
    ox_gather<ND, GDIM>(dd, ut, t);
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
      for (int d = 0; d < GDIM; ++d) w[i][d] -= t[i][d];
  }
}

template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_drag_sigma(int64_t n_cells, const int32_t *__restrict__ vdofs, int64_t n_zone,
                                                    const int32_t *__restrict__ zone_cells, const double *__restrict__ alpha,
                                                    const double *__restrict__ beta, const double *__restrict__ uab,
                                                    const double *__restrict__ ut, double *__restrict__ sigma) {
  using E = Drag<GDIM, DEG>;
  constexpr int ND = E::ND;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_zone) return;
  const int64_t e = zone_cells[k];
  if (e < 0 || e >= n_cells) return;  // a position outside the table reads and writes nothing
  int32_t dd[ND];
  ox_load_dofs<ND>(vdofs, e, dd);
  double w[ND][GDIM];
  drag_gather<GDIM, ND>(dd, uab, ut, w);
  double wc[GDIM] = {};
#pragma unroll
  for (int i = 0; i < ND; ++i)
    if (E::phic(i) != 0.0) {
#pragma unroll
      for (int d = 0; d < GDIM; ++d) wc[d] = fma(w[i][d], E::phic(i), wc[d]);
    }
  double m2 = 0.0;
#pragma unroll
  for (int d = 0; d < GDIM; ++d) m2 = fma(wc[d], wc[d], m2);
  const double mag = sqrt(m2);
  // a velocity that is not finite is shown, not clipped: NaN, whatever beta
  sigma[e] = isfinite(mag) ? fma(beta[k], mag, alpha[k]) : __longlong_as_double(0x7ff8000000000000LL);
}

struct DragRowArgs {
  const double *sigma, *w;
  double *b_first;
  double theta;
};

template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_drag_rows(ox_cells cells, const int32_t *__restrict__ vdofs, ox_adj adj,
                                                   const uint8_t *__restrict__ adj_pos, int64_t n_rows,
                                                   const int64_t *__restrict__ slice_ptr, double *__restrict__ avals,
                                                   const int32_t *__restrict__ slice_list, int n_list, int lds_width,
                                                   DragRowArgs F) {
  using E = Drag<GDIM, DEG>;
  constexpr int ND = E::ND, PW = E::PW, GS = ox_gs(GDIM);
  extern __shared__ double ox_drag_acc[];  // [waves of the block][lds_width][64]: the rows' entries, lane-private columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = blockIdx.x * (int)(blockDim.x >> 6) + wave;
  if (li >= n_list) return;
  const int slice = slice_list[li];
  if (slice < 0 || slice >= adj.n_slices) return;
  const int64_t base = slice_ptr[slice];
  const int width = (int)((slice_ptr[slice + 1] - base) >> 6);
  if (width > lds_width) return;  // (the host lists a slice under a width that holds it; a wider one adds nothing)
  double *__restrict__ acc = ox_drag_acc + (size_t)wave * lds_width * 64 + lane;  // entry k of this lane: acc[k * 64]
  for (int k = 0; k < width; ++k) acc[k * 64] = 0.0;
  const int64_t abase = adj.adj_ptr[slice];
  const int T = (int)((adj.adj_ptr[slice + 1] - abase) >> 6);
  const int64_t row = (int64_t)slice * 64 + lane;
  const double inv_fact = GDIM == 2 ? 0.5 : 1.0 / 6.0;
  const double tm = F.theta;
  double rb[GDIM];
#pragma unroll
  for (int d = 0; d < GDIM; ++d) rb[d] = 0.0;
  bool any = false;  // a row no zone cell touches keeps its bits (-0.0 + 0.0 would not)
  for (int t0 = 0; t0 < T; ++t0) {
    const int64_t pidx = abase + (int64_t)t0 * 64 + lane;
    const int64_t e = adj.adj_cell[pidx];
    if (e < 0 || e >= cells.n_cells) continue;  // padding
    const double s = F.sigma[e];
    if (s == 0.0) continue;  // outside the zones (a NaN is not skipped: it reaches A)
    const int i = adj.adj_loc[pidx];
    if (i >= ND) continue;
    uint8_t pos[PW];
    if constexpr (PW == 32) {
      *reinterpret_cast<uint4 *>(pos) = *reinterpret_cast<const uint4 *>(adj_pos + pidx * 32);
      *reinterpret_cast<uint4 *>(pos + 16) = *reinterpret_cast<const uint4 *>(adj_pos + pidx * 32 + 16);
    } else if constexpr (PW == 16) {
      *reinterpret_cast<uint4 *>(pos) = *reinterpret_cast<const uint4 *>(adj_pos + pidx * 16);
    } else if constexpr (PW == 8) {
      *reinterpret_cast<uint2 *>(pos) = *reinterpret_cast<const uint2 *>(adj_pos + pidx * 8);
    } else {
      *reinterpret_cast<uint32_t *>(pos) = *reinterpret_cast<const uint32_t *>(adj_pos + pidx * 4);
    }
    any = true;
    const double c = s * (ox_geom_adet<GDIM>(cells.geom + (size_t)e * GS) * inv_fact);
    double m[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) m[j] = c * E::mass(i, j);
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const int k = pos[j];
      if (k < width) acc[k * 64] = fma(tm, m[j], acc[k * 64]);  // the slot is private to this lane
    }
    if (F.w) {
      int32_t dd[ND];
      ox_load_dofs<ND>(vdofs, e, dd);
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        const size_t dof = (size_t)dd[j];
#pragma unroll
        for (int d = 0; d < GDIM; ++d) rb[d] = fma(m[j], F.w[dof * GDIM + d], rb[d]);
      }
    }
  }
  if (!any) return;
  // epilogue: the row's entries once, two per 16-byte access as the storage holds them
  typedef double v2d __attribute__((ext_vector_type(2)));
  v2d *__restrict__ av = reinterpret_cast<v2d *>(avals + base) + lane;
  const int npair = width >> 1;
  for (int k = 0; k < npair; ++k) {
    v2d a = av[(size_t)k * 64];
    a.x += acc[(2 * k) * 64];
    a.y += acc[(2 * k + 1) * 64];
    av[(size_t)k * 64] = a;
  }
  if (F.w && row < n_rows) {
#pragma unroll
    for (int d = 0; d < GDIM; ++d) F.b_first[row * GDIM + d] += rb[d];
  }
}

template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_drag_force_cells(ox_cells cells, const int32_t *__restrict__ vdofs, int64_t n_zone,
                                                          const int32_t *__restrict__ zone_cells,
                                                          const double *__restrict__ sigma, const double *__restrict__ u,
                                                          const double *__restrict__ ut, double *__restrict__ ft) {
  using E = Drag<GDIM, DEG>;
  constexpr int ND = E::ND;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_zone) return;
  const int64_t e = zone_cells[k];
  if (e < 0 || e >= cells.n_cells) {  // a position outside the table reads nothing and leaves NaN
#pragma unroll
    for (int d = 0; d < GDIM; ++d) ft[(size_t)k * GDIM + d] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  int32_t dd[ND];
  ox_load_dofs<ND>(vdofs, e, dd);
  double w[ND][GDIM];
  drag_gather<GDIM, ND>(dd, u, ut, w);
  double f[GDIM] = {};
#pragma unroll
  for (int j = 0; j < ND; ++j)
    if (E::colsum(j) != 0.0) {
#pragma unroll
      for (int d = 0; d < GDIM; ++d) f[d] = fma(w[j][d], E::colsum(j), f[d]);
    }
  const double c = sigma[e] * ox_cell_volume<GDIM>(ox_geom_adet<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM)));
#pragma unroll
  for (int d = 0; d < GDIM; ++d) ft[(size_t)k * GDIM + d] = c * f[d];
}

static int drag_zone_check(const char *who, const ox_cells *cells, int64_t n_zone) {
  if (n_zone > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("%s: %lld zone cells, %lld cells", who, (long long)n_zone, (long long)cells->n_cells);
  return 0;
}

}  // namespace

extern "C" int ox_drag_sigma(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_zone,
                             const int32_t *zone_cells, const double *alpha, const double *beta, const double *uab,
                             const double *ut, double *sigma, void *stream) {
  if (!cells || !cell_vdofs || !zone_cells || !alpha || !beta || !uab || !sigma) OX_FAIL("ox_drag_sigma: null argument");
  if (n_zone <= 0) return 0;
  if (drag_zone_check("ox_drag_sigma", cells, n_zone)) return -1;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_zone + 255) / 256);
#define OX_DRAG_SIGMA_CASE(GD, DU)                                                                                   \
  if (g == GD && u_degree == DU) {                                                                                   \
    if (ox_prof_on) ox_prof_start(OX_TAG_DRAG_SIGMA, st, n_zone);                                                    \
    hipLaunchKernelGGL((k_drag_sigma<GD, DU>), dim3(nblk), dim3(256), 0, st, cells->n_cells, cell_vdofs, n_zone,     \
                       zone_cells, alpha, beta, uab, ut, sigma);                                                     \
    if (ox_prof_on) ox_prof_stop(st);                                                                                \
    OX_LAUNCH_CHECK();                                                                                               \
    return 0;                                                                                                        \
  }
  OX_FOR_GDIM_DEG(OX_DRAG_SIGMA_CASE)
#undef OX_DRAG_SIGMA_CASE
  OX_FAIL("ox_drag_sigma: unsupported gdim=%d, P%d", g, u_degree);
}

extern "C" int ox_drag_rows(const ox_cells *cells, const ox_space_info *space, const ox_sell *A, int64_t n_list,
                            const int32_t *slice_list, int lds_width, const double *sigma, double theta, const double *w,
                            double *b_first, void *stream) {
  if (!cells || !cells->geom || !space || !A || !slice_list || !sigma || !b_first) OX_FAIL("ox_drag_rows: null argument");
  if (!space->cell_dofs || !space->adj_pos || !space->adj.adj_ptr || !space->adj.adj_cell || !space->adj.adj_loc ||
      !A->slice_ptr || !A->vals)
    OX_FAIL("ox_drag_rows: null argument");
  if (!(theta >= 0.5 && theta <= 1.0)) OX_FAIL("ox_drag_rows: theta=%g outside [0.5, 1]", theta);
  if (space->adj.n_slices != A->n_slices)
    OX_FAIL("ox_drag_rows: %d slices of the adjacency, %d of the matrix", (int)space->adj.n_slices, (int)A->n_slices);
  if (n_list <= 0) return 0;
  if (n_list > (int64_t)A->n_slices) OX_FAIL("ox_drag_rows: %lld slices listed of %d", (long long)n_list, (int)A->n_slices);
  if (cells->n_cells > (int64_t)0x7fffffff) OX_FAIL("ox_drag_rows: %lld cells", (long long)cells->n_cells);
  if (lds_width < 2 || (lds_width & 1)) OX_FAIL("ox_drag_rows: lds_width=%d (an even row width is expected)", lds_width);
  // wave-private accumulators [lds_width][64]; 4 waves per block unless the rows are so wide that fewer fit into 64 KB
  int nw = 4;
  while (nw > 1 && (size_t)nw * lds_width * 64 * sizeof(double) > 64 * 1024) nw >>= 1;
  const size_t lds = (size_t)nw * lds_width * 64 * sizeof(double);
  if (lds > 160 * 1024) OX_FAIL("ox_drag_rows: row width %d needs %zu B of LDS", lds_width, lds);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim, degree = space->degree;
  const unsigned nblk = (unsigned)((n_list + nw - 1) / nw);
  const DragRowArgs F{sigma, w, b_first, theta};
#define OX_DRAG_ROWS_CASE(GD, DU)                                                                                    \
  if (g == GD && degree == DU) {                                                                                     \
    if (space->pw != Drag<GD, DU>::PW || space->adj.nd != Drag<GD, DU>::ND)                                          \
      OX_FAIL("ox_drag_rows: adj_pos stride %d, %d dofs per cell; expected %d, %d", (int)space->pw, (int)space->adj.nd, \
              Drag<GD, DU>::PW, Drag<GD, DU>::ND);                                                                   \
    if (lds > 32 * 1024)                                                                                             \
      OX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_drag_rows<GD, DU>),                               \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                             \
    if (ox_prof_on) ox_prof_start(OX_TAG_DRAG_ROWS, st, n_list);                                                     \
    hipLaunchKernelGGL((k_drag_rows<GD, DU>), dim3(nblk), dim3(64u * nw), lds, st, *cells, space->cell_dofs,         \
                       space->adj, space->adj_pos, A->n_rows, A->slice_ptr, A->vals, slice_list, (int)n_list,        \
                       lds_width, F);                                                                                \
    if (ox_prof_on) ox_prof_stop(st);                                                                                \
    OX_LAUNCH_CHECK();                                                                                               \
    return 0;                                                                                                        \
  }
  OX_FOR_GDIM_DEG(OX_DRAG_ROWS_CASE)
#undef OX_DRAG_ROWS_CASE
  OX_FAIL("ox_drag_rows: unsupported gdim=%d, P%d", g, degree);
}

extern "C" int ox_drag_force_cells(int u_degree, const ox_cells *cells, const int32_t *cell_vdofs, int64_t n_zone,
                                   const int32_t *zone_cells, const double *sigma, const double *u, const double *ut,
                                   double *ft, void *stream) {
  if (!cells || !cells->geom || !cell_vdofs || !zone_cells || !sigma || !u || !ft)
    OX_FAIL("ox_drag_force_cells: null argument");
  if (n_zone <= 0) return 0;
  if (drag_zone_check("ox_drag_force_cells", cells, n_zone)) return -1;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_zone + 255) / 256);
#define OX_DRAG_FORCE_CASE(GD, DU)                                                                                    \
  if (g == GD && u_degree == DU) {                                                                                    \
    if (ox_prof_on) ox_prof_start(OX_TAG_DRAG_FORCE_CELLS, st, n_zone);                                               \
    hipLaunchKernelGGL((k_drag_force_cells<GD, DU>), dim3(nblk), dim3(256), 0, st, *cells, cell_vdofs, n_zone,        \
                       zone_cells, sigma, u, ut, ft);                                                                 \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_DRAG_FORCE_CASE)
#undef OX_DRAG_FORCE_CASE
  OX_FAIL("ox_drag_force_cells: unsupported gdim=%d, P%d", g, u_degree);
}
