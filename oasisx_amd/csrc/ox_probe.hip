// Point evaluation of Lagrange fields: a cell locator, the evaluation at located points and the sampling of probes into a
// device-resident ring (the counterpart of dolfinx.geometry + Function.eval for the oasisx callers).
//
// Locator.  A uniform background grid over the bounding box of the (selected) straight simplices, about one cell per bin;
// per bin the list of the cells whose bounding box, grown by the tolerance, overlaps it: a count pass, an exclusive scan,
// a fill pass with integer cursors and a sort of every segment -- the lists come out ASCENDING in cell position whatever
// the launch order.  ``find`` takes one lane per point: bin of the point, walk the bin's list, barycentric coordinates
// lambda_a = grad(lambda_a) . (x - x_0) (a = 1..d; the rows of fem.cell_geometry), lambda_0 = 1 - sum; the point is in the
// cell when min lambda >= -tol.  The first hit of the ascending list is the LOWEST containing cell: the same answer on
// every run, for points on shared faces too.  Points outside the grid's box return -1 without touching memory.
//
// Evaluation.  One lane per point, the points sorted by kernel-cell position by the caller (the cell order is the tiled
// spatial order of the mat-vecs: the lanes of a wave open neighbouring rows of the field): gather the cell's dof rows,
// evaluate the basis in barycentric form (P1, P2, the gll_warped P3 element through its monomial coefficients in
// __constant__ memory), accumulate in dof order, write out[perm[i]].  No atomics on doubles, no LDS, nothing read back.
#include "ox_element.h"

#define OX_P3_COEF_QUAL __constant__
#include "fe_tables_eval.h"

#define OX_LOC_SCAN_ITEMS 8                          // bins per thread of the scan's first pass
#define OX_LOC_SCAN_TILE (256 * OX_LOC_SCAN_ITEMS)   // bins per block
#define OX_LOC_MAX_BINS ((int64_t)1 << 30)

struct LocGrid {
  double lo[3], hi[3], inv_h[3];
  int nb[3];
};

struct ox_locator {
  int gdim;
  int64_t n_cells;   // cells in the grid (the selection, or all cells of the mesh)
  int64_t n_bins, n_list;
  double tol;
  LocGrid grid;
  void *mem;         // x0, grad, box
  void *mem_grid;    // bin_ptr, cursor
  void *mem_list;
  double *x0;        // [n_cells][d]   first vertex
  double *grad;      // [n_cells][d*d] grad(lambda_1..d), the rows of fem.cell_geometry
  double *box;       // [n_cells][2d]  bounding box grown by the tolerance
  int64_t *ids;      // [n_cells] mesh cell id of position i, ascending (nullptr: position = id)
  int64_t *bin_ptr;  // [n_bins + 1]
  int32_t *list;     // [n_list] cell positions, ascending inside every bin
};

// ---------------------------------------------------------------------------------------------------------------------
// set-up kernels
// the block's box and the sum of its items' extents: minima, maxima, sums into partial[blockIdx.x][3 D] (a fixed order: the
// sums are the same on every run)
template <int D>
__device__ __forceinline__ void loc_block_box(const double (&mn)[D], const double (&mx)[D], const double (&sm)[D],
                                              double *__restrict__ partial) {
  __shared__ double red[4 * 3 * D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double a = mn[k], b = mx[k], c = sm[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      a = fmin(a, __shfl_down(a, off, 64)), b = fmax(b, __shfl_down(b, off, 64)), c += __shfl_down(c, off, 64);
    if (lane == 0) red[wave * 3 * D + k] = a, red[wave * 3 * D + D + k] = b, red[wave * 3 * D + 2 * D + k] = c;
  }
  __syncthreads();
  if (threadIdx.x < 3 * D) {
    const int k = threadIdx.x;
    double v = red[k];
    for (int w = 1; w < 4; ++w) {
      const double p = red[w * 3 * D + k];
      v = k < D ? fmin(v, p) : (k < 2 * D ? fmax(v, p) : v + p);
    }
    partial[(size_t)blockIdx.x * 3 * D + k] = v;
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_loc_geom(int64_t n, int64_t n_verts, int64_t n_mesh_cells,
                                                  const double *__restrict__ coords, const int64_t *__restrict__ cells,
                                                  const int64_t *__restrict__ ids, double tol, double pad_abs,
                                                  double *__restrict__ x0, double *__restrict__ grad,
                                                  double *__restrict__ box, double *__restrict__ partial) {
  double mn[D], mx[D], sm[D];
#pragma unroll
  for (int k = 0; k < D; ++k) mn[k] = INFINITY, mx[k] = -INFINITY, sm[k] = 0.0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int64_t c = ids ? ids[i] : i;
    double x[D + 1][D];
    bool ok = c >= 0 && c < n_mesh_cells;
#pragma unroll
    for (int a = 0; a <= D; ++a) {
      const int64_t v = ok ? cells[c * (D + 1) + a] : -1;
      ok = ok && v >= 0 && v < n_verts;
#pragma unroll
      for (int k = 0; k < D; ++k) x[a][k] = ok ? coords[v * D + k] : NAN;
    }
    double e[D][D];  // rows = edge vectors x_a - x_0
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int k = 0; k < D; ++k) e[a][k] = x[a + 1][k] - x[0][k];
    double g[D * D];
    if constexpr (D == 2) {
      const double a = e[0][0], b = e[1][0], c2 = e[0][1], dd = e[1][1];  // J = [[a, b], [c2, dd]]
      const double det = a * dd - b * c2;
      g[0] = dd / det, g[1] = -b / det, g[2] = -c2 / det, g[3] = a / det;
    } else {
      const double *e1 = e[0], *e2 = e[1], *e3 = e[D - 1];
      double c23[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
      double c31[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
      double c12[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const double det = e1[0] * c23[0] + e1[1] * c23[1] + e1[2] * c23[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = c23[k] / det, g[3 + k] = c31[k] / det, g[6 + k] = c12[k] / det;
    }
#pragma unroll
    for (int k = 0; k < D * D; ++k) grad[i * D * D + k] = g[k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double l = x[0][k], h = x[0][k];
#pragma unroll
      for (int a = 1; a <= D; ++a) l = fmin(l, x[a][k]), h = fmax(h, x[a][k]);
      // a point with min lambda >= -tol lies within (d + 1) tol cell extents of the hull
      const double pad = (D + 2) * tol * (h - l) + 1e-15 * fmax(fabs(l), fabs(h)) + pad_abs;
      l -= pad, h += pad;
      x0[i * D + k] = x[0][k];
      box[i * 2 * D + k] = l, box[i * 2 * D + D + k] = h;
      if (ok) mn[k] = l, mx[k] = h, sm[k] = h - l;
    }
  }
  loc_block_box<D>(mn, mx, sm, partial);
}

// out[k] = min (k < D) / max (D <= k < 2 D) / sum (k >= 2 D) over the blocks' partial records; one block
template <int D>
__global__ __launch_bounds__(256) void k_loc_box(const double *__restrict__ partial, int nblk, double *__restrict__ out) {
  __shared__ double red[256];
  for (int k = 0; k < 3 * D; ++k) {
    double v = k < D ? INFINITY : (k < 2 * D ? -INFINITY : 0.0);
    for (int b = threadIdx.x; b < nblk; b += 256) {
      const double p = partial[(size_t)b * 3 * D + k];
      v = k < D ? fmin(v, p) : (k < 2 * D ? fmax(v, p) : v + p);
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        const double p = red[threadIdx.x + s];
        red[threadIdx.x] = k < D ? fmin(red[threadIdx.x], p) : (k < 2 * D ? fmax(red[threadIdx.x], p) : red[threadIdx.x] + p);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = red[0];
    __syncthreads();
  }
}

// bin index along axis k of a coordinate inside [lo, hi]; monotone in x, so lo_cell <= x <= hi_cell puts the point's bin
// inside the cell's bin range
__device__ __forceinline__ int loc_bin(const LocGrid &G, int k, double x) {
  const double t = (x - G.lo[k]) * G.inv_h[k];
  int b = t > 0.0 ? (t < 2.0e9 ? (int)t : G.nb[k] - 1) : 0;
  return b < G.nb[k] ? b : G.nb[k] - 1;
}

// pass 0: counts (cursor[bin] += 1); pass 1: fill (list[bin_ptr[bin] + cursor[bin]++] = cell)
template <int D, int FILL>
__global__ __launch_bounds__(256) void k_loc_bins(int64_t n, LocGrid G, const double *__restrict__ box, int64_t n_bins,
                                                  const int64_t *__restrict__ bin_ptr, int *__restrict__ cursor,
                                                  int32_t *__restrict__ list, int64_t n_list) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double l = box[i * 2 * D + k], h = box[i * 2 * D + D + k];
    if (!(l <= h)) return;  // (a cell with an invalid vertex: in no bin)
    b0[k] = loc_bin(G, k, l), b1[k] = loc_bin(G, k, h);
  }
  for (int z = b0[2]; z <= b1[2]; ++z)
    for (int y = b0[1]; y <= b1[1]; ++y)
      for (int x = b0[0]; x <= b1[0]; ++x) {
        const int64_t bin = ((int64_t)z * G.nb[1] + y) * G.nb[0] + x;
        if (bin < 0 || bin >= n_bins) continue;
        const int slot = atomicAdd(&cursor[bin], 1);
        if (FILL) {
          const int64_t at = bin_ptr[bin] + slot;
          if (at >= 0 && at < bin_ptr[bin + 1] && at < n_list) list[at] = (int32_t)i;
        }
      }
}

// exclusive scan of int counts into int64 offsets, three passes
__global__ __launch_bounds__(256) void k_loc_scan_tiles(int64_t n, const int *__restrict__ cnt, int64_t *__restrict__ off,
                                                        int64_t *__restrict__ tile_sum) {
  __shared__ int64_t sh[256];
  const int64_t base = (int64_t)blockIdx.x * OX_LOC_SCAN_TILE + (int64_t)threadIdx.x * OX_LOC_SCAN_ITEMS;
  int64_t v[OX_LOC_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int j = 0; j < OX_LOC_SCAN_ITEMS; ++j) {
    v[j] = s;
    s += base + j < n ? (int64_t)cnt[base + j] : 0;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the thread sums
    const int64_t t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  const int64_t excl = sh[threadIdx.x] - s;
#pragma unroll
  for (int j = 0; j < OX_LOC_SCAN_ITEMS; ++j)
    if (base + j < n) off[base + j] = excl + v[j];
  if (threadIdx.x == 255) tile_sum[blockIdx.x] = sh[255];
}
__global__ __launch_bounds__(64) void k_loc_scan_sums(int64_t ntiles, int64_t *__restrict__ tile_sum, int64_t *__restrict__ total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t s = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t v = tile_sum[t];
    tile_sum[t] = s;
    s += v;
  }
  *total = s;
}
__global__ __launch_bounds__(256) void k_loc_scan_add(int64_t n, int64_t *__restrict__ off, const int64_t *__restrict__ tile_sum,
                                                      const int64_t *__restrict__ total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) off[i] += tile_sum[i / OX_LOC_SCAN_TILE];
  if (i == n) off[n] = *total;
}

// one lane per bin: insertion sort of the bin's segment (a few tens of entries)
__global__ __launch_bounds__(256) void k_loc_sort(int64_t n_bins, const int64_t *__restrict__ bin_ptr, int32_t *__restrict__ list,
                                                  int64_t n_list) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= n_bins) return;
  const int64_t s0 = bin_ptr[b], s1 = bin_ptr[b + 1];
  if (s0 < 0 || s1 > n_list) return;
  for (int64_t i = s0 + 1; i < s1; ++i) {
    const int32_t v = list[i];
    int64_t j = i;
    while (j > s0 && list[j - 1] > v) {
      list[j] = list[j - 1];
      --j;
    }
    list[j] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// queries
template <int D>
__device__ __forceinline__ double loc_bary(const double *__restrict__ x0, const double *__restrict__ grad, int64_t c,
                                           const double (&x)[D], double (&lam)[D + 1]) {
  double r[D], l0 = 1.0;
#pragma unroll
  for (int k = 0; k < D; ++k) r[k] = x[k] - x0[c * D + k];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(grad[c * D * D + a * D + k], r[k], s);
    lam[a + 1] = s;
    l0 -= s;
  }
  lam[0] = l0;
  double m = l0;
#pragma unroll
  for (int a = 1; a <= D; ++a) m = fmin(m, lam[a]);
  return m;
}

template <int D>
__global__ __launch_bounds__(256) void k_loc_find(int64_t n, const double *__restrict__ xs, LocGrid G, int64_t n_cells,
                                                  int64_t n_bins, const int64_t *__restrict__ bin_ptr,
                                                  const int32_t *__restrict__ list, int64_t n_list,
                                                  const double *__restrict__ x0, const double *__restrict__ grad,
                                                  const int64_t *__restrict__ ids, double tol, int64_t *__restrict__ cell_out,
                                                  double *__restrict__ bary_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x[D];
  bool inside = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = xs[i * D + k];
    inside = inside && (x[k] >= G.lo[k]) && (x[k] <= G.hi[k]);  // (NaN: outside)
  }
  int64_t found = -1;
  double lam[D + 1];
#pragma unroll
  for (int a = 0; a <= D; ++a) lam[a] = NAN;
  if (inside) {
    int64_t bin = 0;
#pragma unroll
    for (int k = D - 1; k >= 0; --k) bin = bin * G.nb[k] + loc_bin(G, k, x[k]);
    if (bin >= 0 && bin < n_bins) {
      int64_t s0 = bin_ptr[bin], s1 = bin_ptr[bin + 1];
      if (s0 < 0) s0 = 0;
      if (s1 > n_list) s1 = n_list;
      for (int64_t s = s0; s < s1; ++s) {
        const int64_t c = list[s];
        if (c < 0 || c >= n_cells) continue;
        double l[D + 1];
        if (loc_bary<D>(x0, grad, c, x, l) >= -tol) {  // ascending list: the first hit is the lowest containing cell
          found = c;
#pragma unroll
          for (int a = 0; a <= D; ++a) lam[a] = l[a];
          break;
        }
      }
    }
  }
  cell_out[i] = found < 0 ? -1 : (ids ? ids[found] : found);
#pragma unroll
  for (int a = 0; a <= D; ++a) bary_out[i * (D + 1) + a] = lam[a];
}

// barycentric coordinates of points in GIVEN cells (mesh cell ids; -1 or a cell outside the locator: NaN)
template <int D>
__global__ __launch_bounds__(256) void k_loc_bary(int64_t n, const double *__restrict__ xs, const int64_t *__restrict__ cells,
                                                  int64_t n_cells, const double *__restrict__ x0, const double *__restrict__ grad,
                                                  const int64_t *__restrict__ ids, double *__restrict__ bary_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cells[i];
  int64_t pos = -1;
  if (!ids) {
    pos = c >= 0 && c < n_cells ? c : -1;
  } else if (c >= 0) {  // ids ascending: binary search
    int64_t a = 0, b = n_cells;
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (ids[m] < c) a = m + 1;
      else b = m;
    }
    if (a < n_cells && ids[a] == c) pos = a;
  }
  double lam[D + 1];
#pragma unroll
  for (int a = 0; a <= D; ++a) lam[a] = NAN;
  if (pos >= 0) {
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xs[i * D + k];
    loc_bary<D>(x0, grad, pos, x, lam);
  }
#pragma unroll
  for (int a = 0; a <= D; ++a) bary_out[i * (D + 1) + a] = lam[a];
}

// ---------------------------------------------------------------------------------------------------------------------
// evaluation

// phi of the P1 / P2 element of fem.lagrange_basis at the barycentric point lam
template <int D, int DEG>
__device__ __forceinline__ void probe_basis(const double (&lam)[D + 1], double (&phi)[ox_nd(D, DEG)]) {
  if constexpr (DEG == 1) {
#pragma unroll
    for (int a = 0; a <= D; ++a) phi[a] = lam[a];
  } else {
#pragma unroll
    for (int a = 0; a <= D; ++a) phi[a] = lam[a] * (2.0 * lam[a] - 1.0);
    if constexpr (D == 2) {  // local_edges(2): (1, 2), (0, 2), (0, 1)
      phi[3] = 4.0 * lam[1] * lam[2], phi[4] = 4.0 * lam[0] * lam[2], phi[5] = 4.0 * lam[0] * lam[1];
    } else {  // local_edges(3): (2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)
      phi[4] = 4.0 * lam[2] * lam[3], phi[5] = 4.0 * lam[1] * lam[3], phi[6] = 4.0 * lam[1] * lam[2];
      phi[7] = 4.0 * lam[0] * lam[3], phi[8] = 4.0 * lam[0] * lam[2], phi[9] = 4.0 * lam[0] * lam[1];
    }
  }
}
// the monomials of fem._p3_mono at lam: m_c = lambda_1^i lambda_2^j [lambda_3^k], exponents with i slowest
template <int D>
__device__ __forceinline__ void probe_mono3(const double (&lam)[D + 1], double (&m)[ox_nd(D, 3)]) {
  double p[D][4];
#pragma unroll
  for (int v = 0; v < D; ++v) {
    p[v][0] = 1.0, p[v][1] = lam[v + 1];
    p[v][2] = p[v][1] * p[v][1], p[v][3] = p[v][2] * p[v][1];
  }
  int c = 0;
  if constexpr (D == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4 - i; ++j) m[c++] = p[0][i] * p[1][j];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4 - i; ++j)
#pragma unroll
        for (int k = 0; k < 4 - i - j; ++k) m[c++] = p[0][i] * p[1][j] * p[D - 1][k];
  }
}
// phi_a of the gll_warped P3 element from the monomials: column a of the coefficient matrix (a uniform over the wave: the
// coefficients arrive by scalar loads)
template <int D>
__device__ __forceinline__ double probe_phi3(const double (&m)[ox_nd(D, 3)], int a) {
  constexpr int ND = ox_nd(D, 3);
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    if constexpr (D == 2) s = fma(m[q], OX_P3_COEF2[q][a], s);
    else s = fma(m[q], OX_P3_COEF3[q][a], s);
  }
  return s;
}

// out[perm[i] * ld + v] = sum_a phi_a(bary_i) field[cell_dofs[pos_i][a]][col0 + v], v < nv; a point without a cell: NaN
template <int D, int DEG>
__global__ __launch_bounds__(256) void k_eval_points(int64_t n, const int32_t *__restrict__ cell_dofs, int64_t n_cells,
                                                     int64_t n_rows, const int64_t *__restrict__ cell_pos,
                                                     const double *__restrict__ bary, const int64_t *__restrict__ perm,
                                                     const double *__restrict__ field, int nc, int col0, int nv,
                                                     double *__restrict__ out, int64_t ld) {
  constexpr int ND = ox_nd(D, DEG);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t dst = perm ? perm[i] : i;
  if (dst < 0 || dst >= n) return;
  const int64_t c = cell_pos[i];
  double acc[OX_MAXC];
#pragma unroll
  for (int v = 0; v < OX_MAXC; ++v) acc[v] = 0.0;
  bool ok = c >= 0 && c < n_cells;
  if (ok) {
    double lam[D + 1];
#pragma unroll
    for (int a = 0; a <= D; ++a) lam[a] = bary[i * (D + 1) + a];
    auto add = [&](int a, double phi_a) {
      const int64_t r = cell_dofs[c * ND + a];
      if (r < 0 || r >= n_rows) {
        ok = false;
        return;
      }
      const double *row = field + r * nc + col0;
#pragma unroll
      for (int v = 0; v < OX_MAXC; ++v)
        if (v < nv) acc[v] = fma(phi_a, row[v], acc[v]);
    };
    if constexpr (DEG < 3) {
      double phi[ND];
      probe_basis<D, DEG>(lam, phi);
#pragma unroll
      for (int a = 0; a < ND; ++a) add(a, phi[a]);
    } else {
      double m[ND];
      probe_mono3<D>(lam, m);
#pragma unroll 2
      for (int a = 0; a < ND; ++a) add(a, probe_phi3<D>(m, a));
    }
  }
#pragma unroll
  for (int v = 0; v < OX_MAXC; ++v)
    if (v < nv) out[dst * ld + v] = ok ? acc[v] : NAN;
}

// ---------------------------------------------------------------------------------------------------------------------
// Lagrangian tracers: one lane carries one particle through a whole time step (all substeps, all Runge-Kutta stages) in
// registers.  Per stage: the cached cell is tested (hint) or the point walks its bin's list exactly as k_loc_find does;
// the basis is formed and the dof rows of BOTH time levels are gathered in dof order; the blend
// v = fma(theta, u_b - u_a, u_a) gives the stage velocity.  A particle whose stage point -- or whose end point, which is
// the next substep's first stage point -- lies in no cell is frozen at the start of that substep (status 1); a non-finite
// velocity or an index out of range freezes it the same way with status 2.  No LDS, no atomics, no cross-lane traffic;
// every loop is bounded by substeps, the stage count or a clamped list range.
struct TracerParams {
  LocGrid G;
  int64_t n_loc, n_bins, n_list;
  const int64_t *bin_ptr;
  const int32_t *list;
  const double *x0, *grad;
  const int32_t *cell_dofs;
  int64_t n_cells, n_rows;
  const int64_t *cell_inv;
  const double *u_a, *u_b;
  int nc;
  double t, dt, tol;
  int substeps, scheme, use_hint;
  int64_t n;
  double *x;
  int64_t *cell;
  int32_t *status;
  double *age, *path, *t_exit;
};

// the time of the substep's start, t + theta_s dt, as a product and a sum rounded separately (the numpy model's form)
__device__ __forceinline__ double tracer_exit_time(double t, double theta_s, double dt) {
#pragma clang fp contract(off)
  const double p = theta_s * dt;
  return t + p;
}

// the cell of x: the cached `cell` when the hint is on and all its barycentric coordinates are >= 0, else the lowest
// containing cell of the bin's list (lambda >= -tol); false: none (outside the grid's box, NaN, or in no listed cell)
template <int D>
__device__ __forceinline__ bool tracer_locate(const TracerParams &P, const double (&x)[D], int64_t &cell, double (&lam)[D + 1]) {
  if (P.use_hint && cell >= 0 && cell < P.n_loc && loc_bary<D>(P.x0, P.grad, cell, x, lam) >= 0.0) return true;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < D; ++k) inside = inside && (x[k] >= P.G.lo[k]) && (x[k] <= P.G.hi[k]);  // (NaN: outside)
  if (!inside) return false;
  int64_t bin = 0;
#pragma unroll
  for (int k = D - 1; k >= 0; --k) bin = bin * P.G.nb[k] + loc_bin(P.G, k, x[k]);
  if (bin < 0 || bin >= P.n_bins) return false;
  int64_t s0 = P.bin_ptr[bin], s1 = P.bin_ptr[bin + 1];
  if (s0 < 0) s0 = 0;
  if (s1 > P.n_list) s1 = P.n_list;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t c = P.list[s];
    if (c < 0 || c >= P.n_loc) continue;
    if (loc_bary<D>(P.x0, P.grad, c, x, lam) >= -P.tol) {  // ascending list: the first hit is the lowest containing cell
      cell = c;
      return true;
    }
  }
  return false;
}

// v = (1 - theta) u_a(x) + theta u_b(x) in mesh cell `cell` at the barycentric point lam; false: an index out of range or
// a non-finite value
template <int D, int DEG>
__device__ __forceinline__ bool tracer_velocity(const TracerParams &P, int64_t cell, const double (&lam)[D + 1], double theta,
                                                double (&v)[D]) {
  constexpr int ND = ox_nd(D, DEG);
  const int64_t kp = P.cell_inv[cell];  // (cell is in [0, n_loc) = [0, n_mesh_cells): the caller's check)
  if (kp < 0 || kp >= P.n_cells) return false;
  double ua[D], ub[D];
#pragma unroll
  for (int k = 0; k < D; ++k) ua[k] = 0.0, ub[k] = 0.0;
  bool ok = true;
  auto add = [&](int a, double phi_a) {
    const int64_t r = P.cell_dofs[kp * ND + a];
    if (r < 0 || r >= P.n_rows) {
      ok = false;
      return;
    }
    const double *ra = P.u_a + r * P.nc, *rb = P.u_b + r * P.nc;
#pragma unroll
    for (int k = 0; k < D; ++k) ua[k] = fma(phi_a, ra[k], ua[k]), ub[k] = fma(phi_a, rb[k], ub[k]);
  };
  if constexpr (DEG < 3) {
    double phi[ND];
    probe_basis<D, DEG>(lam, phi);
#pragma unroll
    for (int a = 0; a < ND; ++a) add(a, phi[a]);
  } else {
    double m[ND];
    probe_mono3<D>(lam, m);
#pragma unroll 2
    for (int a = 0; a < ND; ++a) add(a, probe_phi3<D>(m, a));
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    v[k] = fma(theta, ub[k] - ua[k], ua[k]);
    ok = ok && isfinite(v[k]);
  }
  return ok;
}

template <int D, int DEG>
__global__ __launch_bounds__(256) void k_tracer_advance(TracerParams P) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  if (P.status[i] != 0) return;
  double x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = P.x[i * D + k];
  int64_t cell = P.cell[i];
  double age = P.age[i], path = P.path[i], t_exit = P.t_exit[i];
  const double m = (double)P.substeps, h = P.dt / m;
  const int n_stages = P.scheme == 0 ? 1 : (P.scheme == 1 ? 2 : 4);
  const double scale = P.scheme == 2 ? h / 6.0 : h;
  int status = 0;
  for (int s = 0; s < P.substeps && status == 0; ++s) {
    // stage j: point x + a_j h k_{j-1} at theta = (s + a_j) / m, a = (0, 1/2, 1/2, 1); x_new = x + scale * sum_j w_j k_j with
    // w = (1) [Euler], (0, 1) [midpoint], (1, 2, 2, 1) [RK4]
    double ks[D], kj[D], xs[D], lam[D + 1];
#pragma unroll
    for (int k = 0; k < D; ++k) ks[k] = 0.0, kj[k] = 0.0, xs[k] = x[k];
    for (int j = 0; j < n_stages && status == 0; ++j) {
      const double a = j == 0 ? 0.0 : (j == 3 ? 1.0 : 0.5);
      const double w = P.scheme == 0 ? 1.0 : (P.scheme == 1 ? (double)j : (j == 0 || j == 3 ? 1.0 : 2.0));
      if (j == 0) {  // the substep's start lies in `cell`: the seed's location, or the location of the last end point
        if (cell < 0 || cell >= P.n_loc) status = 2;
        else loc_bary<D>(P.x0, P.grad, cell, xs, lam);
      } else {
#pragma unroll
        for (int k = 0; k < D; ++k) xs[k] = fma(a * h, kj[k], x[k]);
        if (!tracer_locate<D>(P, xs, cell, lam)) status = 1;
      }
      if (status == 0) {
        if (!tracer_velocity<D, DEG>(P, cell, lam, ((double)s + a) / m, kj)) status = 2;
#pragma unroll
        for (int k = 0; k < D; ++k) ks[k] = fma(w, kj[k], ks[k]);
      }
    }
    if (status == 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) xs[k] = fma(scale, ks[k], x[k]);
      if (!tracer_locate<D>(P, xs, cell, lam)) status = 1;
    }
    if (status == 0) {
      double d2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double d = xs[k] - x[k];
        d2 = fma(d, d, d2);
        x[k] = xs[k];
      }
      path += sqrt(d2);
      age += h;
    } else {
      t_exit = tracer_exit_time(P.t, (double)s / m, P.dt);
      cell = -1;
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) P.x[i * D + k] = x[k];
  P.cell[i] = cell;
  P.status[i] = status;
  P.age[i] = age, P.path[i] = path, P.t_exit[i] = t_exit;
}

// ---------------------------------------------------------------------------------------------------------------------
// Inertial particles: dx/dt = v, dv/dt = (f / tau_p)(u(x, t) - v) + beta g, one lane per particle,
// all substeps and both stages in registers, the tracers' locate / gather / blend.  A substep of h from (x, v) at theta_s
// freezes the drag factor f (1, or Schiller-Naumann's 1 + 0.15 Re_p^0.687 of the start) and the fluid velocity
// (exp1: of the start; exp2: of the exponential half step's end at theta_s + 1 / (2 substeps)) and integrates the linear
// equation exactly: with tau_e = tau_p / f, w = u + tau_e beta g, E = exp(-h / tau_e), phi = tau_e (1 - E) [as -expm1],
//   x_new = x + h w + phi (v - w),  v_new = w + E (v - w);   tau_e == 0: E = phi = 0 (the tracers' Euler / midpoint rule).
// Every predictor and end point is folded into [lo, hi) on the periodic axes before it is located; the image counts go to
// wraps.  A point in no cell freezes the particle at the substep's start with status 1 exactly as a tracer, and the
// (folded) point goes to xq with facet = -2: k_particle_classify, the second launch, names its nearest exterior facet.
// No LDS, no atomics, no cross-lane traffic; every loop is bounded by substeps or a clamped list range.
#define OX_PARTICLE_PENDING (-2)
struct ParticleParams {
  double *v;          // [n][D]
  int32_t *wraps;     // [n][D]
  int32_t *facet;     // [n]
  double *xq;         // [n][D] the point that left, for the classification
  const double *tau_p, *diam, *beta;  // [n]
  double g[3], nu;
  int drag;
  int periodic[3];
  double lo[3], hi[3], period[3];
};

// x folded into [lo, hi) on the periodic axes (the fold of k_dyn_lagrangian); w: the images it went through
template <int D>
__device__ __forceinline__ void particle_fold(const ParticleParams &A, double (&x)[D], int (&w)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    w[k] = 0;
    if (A.periodic[k]) {
      const double q = floor((x[k] - A.lo[k]) / A.period[k]);
      double xk = x[k] - A.period[k] * q;
      int n = (q >= -2147483647.0 && q <= 2147483647.0) ? (int)q : 0;  // (a non-finite x: caught by the caller)
      if (xk >= A.hi[k]) xk -= A.period[k], n += 1;
      x[k] = xk, w[k] = n;
    }
  }
}

// E = exp(-h / tau_e), phi = tau_e (1 - E); tau_e == 0: both 0
__device__ __forceinline__ void particle_coef(double h, double tau_e, double &E, double &phi) {
  E = 0.0, phi = 0.0;
  if (tau_e != 0.0) {
    const double r = h / tau_e;
    E = exp(-r);
    phi = tau_e * (-expm1(-r));
  }
}

template <int D, int DEG>
__global__ __launch_bounds__(256) void k_particle_advance(TracerParams P, ParticleParams A) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  if (P.status[i] != 0) return;
  double x[D], v[D], g[D];
  int wraps[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = P.x[i * D + k], v[k] = A.v[i * D + k], wraps[k] = A.wraps[i * D + k], g[k] = A.g[k];
  int64_t cell = P.cell[i];
  double age = P.age[i], path = P.path[i], t_exit = P.t_exit[i];
  const double tau_p = A.tau_p[i], diam = A.diam[i], beta = A.beta[i];
  const double m = (double)P.substeps, h = P.dt / m;
  int status = 0;
  double xs[D];  // the point of the last move: the one that left, where the status becomes 1
#pragma unroll
  for (int k = 0; k < D; ++k) xs[k] = x[k];
  const int n_stages = P.scheme == 1 ? 2 : 1;
  for (int s = 0; s < P.substeps && status == 0; ++s) {
    // point j: 0 the start (in `cell`), 0 < j < n_stages the exponential half step's end, j == n_stages the end point; every
    // point but the start is folded and located, every point but the end gives the fluid velocity of the next move
    double u[D], w[D], xu[D], vn[D], lam[D + 1];
    int ws[D];
#pragma unroll
    for (int k = 0; k < D; ++k) w[k] = 0.0, xu[k] = x[k], vn[k] = v[k], ws[k] = 0;
    double tg = 0.0, tau_e = 0.0;
    for (int j = 0; j <= n_stages && status == 0; ++j) {
      if (j == 0) {
        if (cell < 0 || cell >= P.n_loc) status = 2;
        else loc_bary<D>(P.x0, P.grad, cell, x, lam);
      } else {
        const double hq = j == n_stages ? h : 0.5 * h;
        double E, phi;
        particle_coef(hq, tau_e, E, phi);
        bool finite = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double dv = v[k] - w[k];
          xu[k] = fma(phi, dv, fma(hq, w[k], x[k]));
          vn[k] = fma(E, dv, w[k]);
          xs[k] = xu[k];
          finite = finite && isfinite(xu[k]) && isfinite(vn[k]);
        }
        if (!finite) status = 2;
        else {
          particle_fold<D>(A, xs, ws);
          if (!tracer_locate<D>(P, xs, cell, lam)) status = 1;
        }
      }
      if (status == 0 && j < n_stages) {
        if (!tracer_velocity<D, DEG>(P, cell, lam, ((double)s + (j == 0 ? 0.0 : 0.5)) / m, u)) status = 2;
        else {
          if (j == 0) {  // the drag factor of the substep's start, frozen over the substep
            double f = 1.0;
            if (A.drag == 1) {
              double r2 = 0.0;
#pragma unroll
              for (int k = 0; k < D; ++k) {
                const double d = u[k] - v[k];
                r2 = fma(d, d, r2);
              }
              f = fma(0.15, pow(diam * sqrt(r2) / A.nu, 0.687), 1.0);
            }
            tau_e = tau_p / f;
            tg = tau_e * beta;
          }
#pragma unroll
          for (int k = 0; k < D; ++k) w[k] = fma(tg, g[k], u[k]);
        }
      }
    }
    if (status == 0) {
      double d2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double d = xu[k] - x[k];  // (the unfolded step)
        d2 = fma(d, d, d2);
        x[k] = xs[k], v[k] = vn[k], wraps[k] += ws[k];
      }
      path += sqrt(d2);
      age += h;
    } else {
      t_exit = tracer_exit_time(P.t, (double)s / m, P.dt);
      cell = -1;
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) P.x[i * D + k] = x[k], A.v[i * D + k] = v[k], A.wraps[i * D + k] = wraps[k];
  P.cell[i] = cell;
  P.status[i] = status;
  P.age[i] = age, P.path[i] = path, P.t_exit[i] = t_exit;
  if (status == 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) A.xq[i * D + k] = xs[k];
    A.facet[i] = OX_PARTICLE_PENDING;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Lagrangian averaging of the dynamic Smagorinsky model: one lane per vertex class traces its path
// line back over h with the patch-mean velocity, x' = x_v - h u_v (folded into the box on periodic axes), finds the cell
// of x' by the tracers' rule (tracer_locate with the patch's first cell as the hint), interpolates the OLD pair
// {F_LM, F_MM} there (P1, local vertex order) and relaxes it towards the sources.  The new pair goes to a second buffer:
// lanes read their neighbours' old values.  No LDS, no atomics, no cross-lane traffic; the only loop is the clamped list
// walk of tracer_locate.
struct LagParams {
  int64_t n;                 // vertex classes
  const double *x;           // [n][D] the master vertex of every class
  const double *u;           // patch-mean velocity: the first D entries of row v
  int64_t u_stride;
  const int64_t *hint;       // [n] mesh cell id of the first cell of the vertex's patch
  const int64_t *cell_inv;   // [n_loc] mesh cell id -> kernel cell position
  int64_t n_cells;
  const int32_t *cell_verts; // [n_cells][D + 1] vertex classes, kernel cell order
  const double *src;         // [n][2] {(LM)_v, (MM)_v}
  const double *delta;       // [n]
  const double *f_old;       // [n][2] {F_LM, F_MM}
  double *f_new;
  double *cs2v;              // [n]
  int32_t *status;           // [n]
  double h, time_scale, cs2_floor, cs2_max, cs2_initial;
  int first;
  int periodic[3];
  double lo[3], hi[3], period[3];
};

// max(a, b) that lets a NaN of either side through
__device__ __forceinline__ double lag_max(double a, double b) { return a >= b ? a : (a != a ? a : b); }

// lm / mm clipped to [0, cmax]; 0 where mm is not positive; a NaN stays a NaN (the comparison forms of dyn_clip)
__device__ __forceinline__ double lag_clip(double lm, double mm, double cmax) {
  if (mm > 0.0) {
    const double c = lm / mm;
    return c < 0.0 ? 0.0 : (c > cmax ? cmax : c);  // (NaN fails both comparisons)
  }
  return (mm != mm || lm != lm) ? (double)NAN : 0.0;
}

template <int D>
__global__ __launch_bounds__(256) void k_dyn_lagrangian(TracerParams L, LagParams A) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= A.n) return;
  const double s_lm = -2.0 * A.src[2 * v], s_mm = 4.0 * A.src[2 * v + 1];
  double f_lm, f_mm;
  int status = 0;
  if (A.first) {
    f_mm = s_mm;
    f_lm = lag_max(A.cs2_initial * s_mm, A.cs2_floor * s_mm);
  } else {
    const double o_lm = A.f_old[2 * v], o_mm = A.f_old[2 * v + 1];
    double xd[D], b_lm = o_lm, b_mm = o_mm;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double xk = fma(-A.h, A.u[v * A.u_stride + k], A.x[v * D + k]);
      finite = finite && isfinite(xk);
      if (A.periodic[k]) {
        xk -= A.period[k] * floor((xk - A.lo[k]) / A.period[k]);
        if (xk >= A.hi[k]) xk -= A.period[k];
      }
      xd[k] = xk;
    }
    int64_t cell = A.hint[v];
    double lam[D + 1];
    if (!finite || cell < 0 || cell >= L.n_loc) status = 2;
    else if (!tracer_locate<D>(L, xd, cell, lam)) status = 1;
    else {
      const int64_t kp = A.cell_inv[cell];  // (cell is in [0, n_loc): tracer_locate's answer)
      if (kp < 0 || kp >= A.n_cells) status = 2;
      else {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int j = 0; j <= D; ++j) {
          const int64_t w = A.cell_verts[kp * (D + 1) + j];
          if (w < 0 || w >= A.n) status = 2;
          else a = fma(lam[j], A.f_old[2 * w], a), b = fma(lam[j], A.f_old[2 * w + 1], b);
        }
        b_lm = a, b_mm = b;
      }
    }
    const double p = o_lm * o_mm;
    double eps = 0.0;
    if (p != p) eps = p;
    else if (p > 0.0 && p < INFINITY) {
      const double T = A.time_scale * A.delta[v] * (1.0 / sqrt(sqrt(sqrt(p))));  // p^(-1/8)
      const double r = A.h / T;
      eps = r / (1.0 + r);
    }
    f_mm = fma(eps, s_mm, (1.0 - eps) * b_mm);
    f_lm = lag_max(fma(eps, s_lm, (1.0 - eps) * b_lm), A.cs2_floor * f_mm);
    if (status == 2) f_lm = f_mm = NAN;
  }
  A.f_new[2 * v] = f_lm;
  A.f_new[2 * v + 1] = f_mm;
  A.cs2v[v] = lag_clip(f_lm, f_mm, A.cs2_max);
  A.status[v] = status;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
static void loc_free(ox_locator *L) {
  if (!L) return;
  if (L->mem) (void)hipFree(L->mem);
  if (L->mem_grid) (void)hipFree(L->mem_grid);
  if (L->mem_list) (void)hipFree(L->mem_list);
  delete L;
}

// Bins per axis, about one item per bin on stretched domains too: r_k = (extent of the box) / (mean extent of an item)
// items span axis k; the bins are r_k scaled by one factor that makes their product n.  (Items of one size on every axis,
// mean_k = m: r_k (n / prod r)^(1/d) = ext_k / (vol / n)^(1/d), the isotropic length.)  hb: minima, maxima and summed
// extents of the n items, [3 D].  bins3 (may be null) overrides the count on every axis that has an extent.
template <int D>
static int loc_size_grid(const char *who, LocGrid &G, const double *hb, int64_t n, const int *bins3, int64_t *n_bins) {
  double r[D], prod = 1.0;
  int nz = 0;
  for (int k = 0; k < D; ++k) {
    if (!(hb[k] <= hb[D + k])) OX_FAIL("%s: the cells have no finite bounding box", who);
    G.lo[k] = hb[k], G.hi[k] = hb[D + k];
    const double ext = G.hi[k] - G.lo[k], mean = hb[2 * D + k] / (double)n;
    r[k] = ext > 0.0 && mean > 0.0 ? ext / mean : 0.0;
    if (!(r[k] >= 1.0)) r[k] = 0.0;  // (a flat or empty axis, or a NaN: one bin)
    if (r[k] > 0.0) prod *= r[k], ++nz;
  }
  const double scale = nz ? pow((double)n / prod, 1.0 / nz) : 1.0;
  int64_t nbins = 1;
  for (int k = 0; k < 3; ++k) G.nb[k] = 1;
  for (int k = 0; k < D; ++k) {
    const double ext = G.hi[k] - G.lo[k];
    double q = r[k] > 0.0 && scale > 0.0 ? ceil(r[k] * scale) : 1.0;
    if (bins3 && ext > 0.0) q = (double)bins3[k];
    if (!(q >= 1.0)) q = 1.0;
    if (q > 1024.0) q = 1024.0;
    G.nb[k] = (int)q;
    G.inv_h[k] = ext > 0.0 ? q / ext : 0.0;
    nbins *= G.nb[k];
  }
  for (int k = D; k < 3; ++k) G.lo[k] = G.hi[k] = G.inv_h[k] = 0.0;
  if (nbins > OX_LOC_MAX_BINS) OX_FAIL("%s: %lld bins", who, (long long)nbins);
  *n_bins = nbins;
  return 0;
}

// Per bin the ASCENDING list of the items whose box [n][2 D] overlaps it: count, scan, fill, sort.  Allocates *mem_grid
// (bin_ptr and the scan's work space) and *mem_list; synchronises the stream.
template <int D>
static int loc_build_lists(const char *who, const LocGrid &G, const double *box, int64_t n, int64_t nbins, hipStream_t st,
                           void **mem_grid, int64_t **bin_ptr_out, void **mem_list, int32_t **list_out,
                           int64_t *n_list_out) {
  const int nblk = (int)((n + 255) / 256);
  const int64_t ntiles = (nbins + OX_LOC_SCAN_TILE - 1) / OX_LOC_SCAN_TILE;
  const size_t gbytes = (size_t)(nbins + 1 + ntiles + 1) * sizeof(int64_t) + (size_t)nbins * sizeof(int);
  if (hipMalloc(mem_grid, gbytes) != hipSuccess) OX_FAIL("%s: hipMalloc of %zu bytes failed", who, gbytes);
  int64_t *bin_ptr = static_cast<int64_t *>(*mem_grid);
  *bin_ptr_out = bin_ptr;
  int64_t *tile_sum = bin_ptr + nbins + 1, *total = tile_sum + ntiles;
  int *cursor = reinterpret_cast<int *>(total + 1);
  OX_HIP(hipMemsetAsync(cursor, 0, (size_t)nbins * sizeof(int), st));
  hipLaunchKernelGGL((k_loc_bins<D, 0>), dim3(nblk), dim3(256), 0, st, n, G, box, nbins, bin_ptr, cursor, nullptr, (int64_t)0);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, st, nbins, cursor, bin_ptr, tile_sum);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_scan_sums, dim3(1), dim3(64), 0, st, ntiles, tile_sum, total);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_scan_add, dim3((unsigned)((nbins + 1 + 255) / 256)), dim3(256), 0, st, nbins, bin_ptr, tile_sum, total);
  OX_LAUNCH_CHECK();
  int64_t n_list = 0;
  OX_HIP(hipMemcpyAsync(&n_list, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  OX_HIP(hipStreamSynchronize(st));
  if (n_list < 0) OX_FAIL("%s: list size %lld", who, (long long)n_list);
  *n_list_out = n_list;
  const size_t lbytes = (size_t)(n_list > 0 ? n_list : 1) * sizeof(int32_t);
  if (hipMalloc(mem_list, lbytes) != hipSuccess) OX_FAIL("%s: hipMalloc of %zu bytes failed", who, lbytes);
  int32_t *list = static_cast<int32_t *>(*mem_list);
  *list_out = list;
  OX_HIP(hipMemsetAsync(list, 0xff, lbytes, st));  // (-1: skipped by the queries)
  OX_HIP(hipMemsetAsync(cursor, 0, (size_t)nbins * sizeof(int), st));
  hipLaunchKernelGGL((k_loc_bins<D, 1>), dim3(nblk), dim3(256), 0, st, n, G, box, nbins, bin_ptr, cursor, list, n_list);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_sort, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, st, nbins, bin_ptr, list, n_list);
  OX_LAUNCH_CHECK();
  OX_HIP(hipStreamSynchronize(st));
  return 0;
}

template <int D>
static int loc_create(ox_locator *L,const double *coords, int64_t n_verts, const int64_t *cells, int64_t n_mesh_cells,
                      const int64_t *ids, double padding, hipStream_t st) {
  const int64_t n = L->n_cells;
  const int nblk = (int)((n + 255) / 256);
  const size_t dbl = (size_t)n * (D + D * D + 2 * D) + (size_t)nblk * 3 * D + 3 * D;
  const size_t bytes = dbl * sizeof(double) + (ids ? (size_t)n * sizeof(int64_t) : 0);
  if (hipMalloc(&L->mem, bytes) != hipSuccess) OX_FAIL("ox_locator_create: hipMalloc of %zu bytes failed", bytes);
  double *p = static_cast<double *>(L->mem);
  L->x0 = p, p += (size_t)n * D;
  L->grad = p, p += (size_t)n * D * D;
  L->box = p, p += (size_t)n * 2 * D;
  double *partial = p;
  p += (size_t)nblk * 3 * D;
  double *gbox = p;
  p += 3 * D;
  if (ids) {
    L->ids = reinterpret_cast<int64_t *>(p);
    OX_HIP(hipMemcpyAsync(L->ids, ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  }
  hipLaunchKernelGGL(k_loc_geom<D>, dim3(nblk), dim3(256), 0, st, n, n_verts, n_mesh_cells, coords, cells, L->ids, L->tol,
                     padding, L->x0, L->grad, L->box, partial);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_box<D>, dim3(1), dim3(256), 0, st, partial, nblk, gbox);
  OX_LAUNCH_CHECK();
  double hb[3 * D];
  OX_HIP(hipMemcpyAsync(hb, gbox, sizeof(hb), hipMemcpyDeviceToHost, st));
  OX_HIP(hipStreamSynchronize(st));
  if (loc_size_grid<D>("ox_locator_create", L->grid, hb, n, nullptr, &L->n_bins)) return -1;
  return loc_build_lists<D>("ox_locator_create", L->grid, L->box, n, L->n_bins, st, &L->mem_grid, &L->bin_ptr, &L->mem_list,
                            &L->list, &L->n_list);
}

extern "C" int ox_locator_create(int gdim, const double *coords, int64_t n_vertices, const int64_t *cells, int64_t n_cells,
                                 const int64_t *cell_ids, int64_t n_ids, double tol, double padding, void *stream,
                                 ox_locator **out) {
  if (!out) OX_FAIL("ox_locator_create: null argument");
  *out = nullptr;
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_locator_create: gdim=%d", gdim);
  if (!coords || !cells || n_vertices < 1 || n_cells < 1) OX_FAIL("ox_locator_create: empty mesh");
  if (!(tol >= 0.0) || !(tol <= 1e-2)) OX_FAIL("ox_locator_create: tol=%g (0..1e-2)", tol);
  if (!(padding >= 0.0)) OX_FAIL("ox_locator_create: padding=%g", padding);
  const int64_t n = cell_ids ? n_ids : n_cells;
  if (n < 1 || n > n_cells || n >= ((int64_t)1 << 31) - 256) OX_FAIL("ox_locator_create: %lld cells selected", (long long)n);
  ox_locator *L = new ox_locator();
  memset(L, 0, sizeof(*L));
  L->gdim = gdim, L->n_cells = n, L->tol = tol;
  hipStream_t st = ox_stream(stream);
  const int rc = gdim == 2 ? loc_create<2>(L, coords, n_vertices, cells, n_cells, cell_ids, padding, st)
                           : loc_create<3>(L, coords, n_vertices, cells, n_cells, cell_ids, padding, st);
  if (rc) {
    loc_free(L);
    return -1;
  }
  *out = L;
  return 0;
}

extern "C" int ox_locator_destroy(ox_locator *L) {
  loc_free(L);
  return 0;
}

extern "C" int ox_locator_info(const ox_locator *L, int64_t *n_cells, int64_t *n_bins, int64_t *n_list, int *bins_per_axis) {
  if (!L) OX_FAIL("ox_locator_info: null handle");
  if (n_cells) *n_cells = L->n_cells;
  if (n_bins) *n_bins = L->n_bins;
  if (n_list) *n_list = L->n_list;
  if (bins_per_axis)
    for (int k = 0; k < 3; ++k) bins_per_axis[k] = L->grid.nb[k];
  return 0;
}

extern "C" int ox_locator_find(const ox_locator *L, int64_t n_points, const double *x, double tol, int64_t *cells, double *bary,
                               void *stream) {
  if (!L || (n_points > 0 && (!x || !cells || !bary))) OX_FAIL("ox_locator_find: null argument");
  if (!(tol >= 0.0) || tol > L->tol) OX_FAIL("ox_locator_find: tol=%g, the grid was built for tol <= %g", tol, L->tol);
  if (n_points <= 0) return 0;
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((n_points + 255) / 256));
  if (L->gdim == 2)
    hipLaunchKernelGGL(k_loc_find<2>, grid, dim3(256), 0, st, n_points, x, L->grid, L->n_cells, L->n_bins, L->bin_ptr, L->list,
                       L->n_list, L->x0, L->grad, L->ids, tol, cells, bary);
  else
    hipLaunchKernelGGL(k_loc_find<3>, grid, dim3(256), 0, st, n_points, x, L->grid, L->n_cells, L->n_bins, L->bin_ptr, L->list,
                       L->n_list, L->x0, L->grad, L->ids, tol, cells, bary);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_locator_bary(const ox_locator *L, int64_t n_points, const double *x, const int64_t *cells, double *bary,
                               void *stream) {
  if (!L || (n_points > 0 && (!x || !cells || !bary))) OX_FAIL("ox_locator_bary: null argument");
  if (n_points <= 0) return 0;
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((n_points + 255) / 256));
  if (L->gdim == 2)
    hipLaunchKernelGGL(k_loc_bary<2>, grid, dim3(256), 0, st, n_points, x, cells, L->n_cells, L->x0, L->grad, L->ids, bary);
  else
    hipLaunchKernelGGL(k_loc_bary<3>, grid, dim3(256), 0, st, n_points, x, cells, L->n_cells, L->x0, L->grad, L->ids, bary);
  OX_LAUNCH_CHECK();
  return 0;
}

static int eval_launch(const char *who, int degree, int gdim, const int32_t *cell_dofs, int64_t n_cells, int64_t n_rows,
                       int64_t n_points, const int64_t *cell_pos, const double *bary, const int64_t *perm, const double *field,
                       int nc, int col, double *out, int64_t ld, int64_t off, hipStream_t st) {
  if (gdim != 2 && gdim != 3) OX_FAIL("%s: gdim=%d", who, gdim);
  if (degree < 1 || degree > 3) OX_FAIL("%s: degree %d (1..3)", who, degree);
  if (nc < 1 || nc > OX_MAXC || col < -1 || col >= nc) OX_FAIL("%s: nc=%d col=%d", who, nc, col);
  const int nv = col < 0 ? nc : 1, col0 = col < 0 ? 0 : col;
  if (off < 0 || ld < off + nv) OX_FAIL("%s: row of %lld values, %d at offset %lld", who, (long long)ld, nv, (long long)off);
  if (n_points <= 0) return 0;
  if (!cell_dofs || !cell_pos || !bary || !field || !out || n_cells < 1 || n_rows < 1) OX_FAIL("%s: null argument", who);
  const dim3 grid((unsigned)((n_points + 255) / 256)), blk(256);
#define OX_EVAL_CASE(D, G)                                                                                              \
  hipLaunchKernelGGL((k_eval_points<D, G>), grid, blk, 0, st, n_points, cell_dofs, n_cells, n_rows, cell_pos, bary, perm, \
                     field, nc, col0, nv, out + off, ld)
  switch (gdim * 10 + degree) {
    case 21: OX_EVAL_CASE(2, 1); break;
    case 22: OX_EVAL_CASE(2, 2); break;
    case 23: OX_EVAL_CASE(2, 3); break;
    case 31: OX_EVAL_CASE(3, 1); break;
    case 32: OX_EVAL_CASE(3, 2); break;
    default: OX_EVAL_CASE(3, 3); break;
  }
#undef OX_EVAL_CASE
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_eval_points(int degree, int gdim, const int32_t *cell_dofs, int64_t n_cells, int64_t n_rows, int64_t n_points,
                              const int64_t *cell_pos, const double *bary, const int64_t *perm, const double *field, int nc,
                              int col, double *out, int64_t ld, int64_t off, void *stream) {
  return eval_launch("ox_eval_points", degree, gdim, cell_dofs, n_cells, n_rows, n_points, cell_pos, bary, perm, field, nc,
                     col, out, ld, off, ox_stream(stream));
}

extern "C" int ox_probe_sample(int degree, int gdim, const int32_t *cell_dofs, int64_t n_cells, int64_t n_rows, int64_t n_points,
                               const int64_t *cell_pos, const double *bary, const int64_t *perm, const double *field, int nc,
                               int col, double *ring, int64_t capacity, int64_t slot, int64_t ld, int64_t off, void *stream) {
  if (n_points <= 0) return 0;
  if (!ring || slot < 0 || slot >= capacity) OX_FAIL("ox_probe_sample: slot %lld of %lld", (long long)slot, (long long)capacity);
  return eval_launch("ox_probe_sample", degree, gdim, cell_dofs, n_cells, n_rows, n_points, cell_pos, bary, perm, field, nc,
                     col, ring + (size_t)slot * (size_t)n_points * (size_t)ld, ld, off, ox_stream(stream));
}

extern "C" int ox_tracer_advance(const ox_tracer_args *a, void *stream) {
  if (!a) OX_FAIL("ox_tracer_advance: null argument (args)");
  if (!a->loc) OX_FAIL("ox_tracer_advance: null argument (loc)");
  if (a->gdim != 2 && a->gdim != 3) OX_FAIL("ox_tracer_advance: gdim=%d", a->gdim);
  if (a->degree < 1 || a->degree > 3) OX_FAIL("ox_tracer_advance: degree %d (1..3)", a->degree);
  if (a->nc < a->gdim || a->nc > OX_MAXC) OX_FAIL("ox_tracer_advance: nc=%d (gdim=%d..%d)", a->nc, a->gdim, OX_MAXC);
  if (a->substeps < 1 || a->substeps > OX_TRACER_MAX_SUBSTEPS)
    OX_FAIL("ox_tracer_advance: substeps=%d (1..%d)", a->substeps, OX_TRACER_MAX_SUBSTEPS);
  if (a->scheme != OX_TRACER_EULER && a->scheme != OX_TRACER_RK2 && a->scheme != OX_TRACER_RK4)
    OX_FAIL("ox_tracer_advance: scheme=%d", a->scheme);
  if (!std::isfinite(a->dt) || !std::isfinite(a->t)) OX_FAIL("ox_tracer_advance: dt=%g at t=%g is not finite", a->dt, a->t);
  const ox_locator *L = a->loc;
  if (L->ids) OX_FAIL("ox_tracer_advance: a locator over a selection of cells; tracers take the whole-mesh locator");
  if (L->gdim != a->gdim) OX_FAIL("ox_tracer_advance: loc->gdim=%d, gdim=%d", L->gdim, a->gdim);
  if (a->n_mesh_cells != L->n_cells)
    OX_FAIL("ox_tracer_advance: n_mesh_cells=%lld, the locator holds %lld", (long long)a->n_mesh_cells, (long long)L->n_cells);
  if (!(a->tol >= 0.0) || a->tol > L->tol) OX_FAIL("ox_tracer_advance: tol=%g, the grid was built for tol <= %g", a->tol, L->tol);
  if (a->n < 0) OX_FAIL("ox_tracer_advance: n=%lld", (long long)a->n);
  if (a->n == 0) return 0;
  if (!a->cell_dofs || !a->cell_inv || !a->u_a || !a->u_b || a->n_cells < 1 || a->n_rows < 1)
    OX_FAIL("ox_tracer_advance: null argument (cell_dofs, cell_inv, u_a, u_b)");
  if (!a->x || !a->cell || !a->status || !a->age || !a->path || !a->t_exit)
    OX_FAIL("ox_tracer_advance: null argument (x, cell, status, age, path, t_exit)");
  TracerParams P;
  P.G = L->grid;
  P.n_loc = L->n_cells, P.n_bins = L->n_bins, P.n_list = L->n_list;
  P.bin_ptr = L->bin_ptr, P.list = L->list, P.x0 = L->x0, P.grad = L->grad;
  P.cell_dofs = a->cell_dofs, P.n_cells = a->n_cells, P.n_rows = a->n_rows, P.cell_inv = a->cell_inv;
  P.u_a = a->u_a, P.u_b = a->u_b, P.nc = a->nc;
  P.t = a->t, P.dt = a->dt, P.tol = a->tol;
  P.substeps = a->substeps, P.scheme = a->scheme, P.use_hint = a->use_hint ? 1 : 0;
  P.n = a->n, P.x = a->x, P.cell = a->cell, P.status = a->status, P.age = a->age, P.path = a->path, P.t_exit = a->t_exit;
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((a->n + 255) / 256)), blk(256);
  switch (a->gdim * 10 + a->degree) {
    case 21: hipLaunchKernelGGL((k_tracer_advance<2, 1>), grid, blk, 0, st, P); break;
    case 22: hipLaunchKernelGGL((k_tracer_advance<2, 2>), grid, blk, 0, st, P); break;
    case 23: hipLaunchKernelGGL((k_tracer_advance<2, 3>), grid, blk, 0, st, P); break;
    case 31: hipLaunchKernelGGL((k_tracer_advance<3, 1>), grid, blk, 0, st, P); break;
    case 32: hipLaunchKernelGGL((k_tracer_advance<3, 2>), grid, blk, 0, st, P); break;
    default: hipLaunchKernelGGL((k_tracer_advance<3, 3>), grid, blk, 0, st, P); break;
  }
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_dynamic_lagrangian(const ox_lagrangian_args *a, void *stream) {
  if (!a) OX_FAIL("ox_dynamic_lagrangian: null argument (args)");
  if (!a->loc) OX_FAIL("ox_dynamic_lagrangian: null argument (loc)");
  if (a->gdim != 2 && a->gdim != 3) OX_FAIL("ox_dynamic_lagrangian: gdim=%d", a->gdim);
  const ox_locator *L = a->loc;
  if (L->ids) OX_FAIL("ox_dynamic_lagrangian: a locator over a selection of cells; the back-trace takes the whole-mesh locator");
  if (L->gdim != a->gdim) OX_FAIL("ox_dynamic_lagrangian: loc->gdim=%d, gdim=%d", L->gdim, a->gdim);
  if (a->n_mesh_cells != L->n_cells)
    OX_FAIL("ox_dynamic_lagrangian: n_mesh_cells=%lld, the locator holds %lld", (long long)a->n_mesh_cells,
            (long long)L->n_cells);
  if (!(a->tol >= 0.0) || a->tol > L->tol)
    OX_FAIL("ox_dynamic_lagrangian: tol=%g, the grid was built for tol <= %g", a->tol, L->tol);
  if (a->n_vertices < 0 || a->n_vertices > (int64_t)0x7fffffff)
    OX_FAIL("ox_dynamic_lagrangian: n_vertices=%lld", (long long)a->n_vertices);
  if (!std::isfinite(a->h) || a->h < 0.0) OX_FAIL("ox_dynamic_lagrangian: h=%g (finite, >= 0)", a->h);
  if (!std::isfinite(a->time_scale) || !(a->time_scale > 0.0)) OX_FAIL("ox_dynamic_lagrangian: time_scale=%g", a->time_scale);
  if (!std::isfinite(a->cs2_max) || a->cs2_max < 0.0) OX_FAIL("ox_dynamic_lagrangian: cs2_max=%g", a->cs2_max);
  if (!(a->cs2_floor >= 0.0) || a->cs2_floor > a->cs2_max)
    OX_FAIL("ox_dynamic_lagrangian: cs2_floor=%g (0..cs2_max=%g)", a->cs2_floor, a->cs2_max);
  if (!std::isfinite(a->cs2_initial) || a->cs2_initial < 0.0) OX_FAIL("ox_dynamic_lagrangian: cs2_initial=%g", a->cs2_initial);
  if (a->u_stride < a->gdim) OX_FAIL("ox_dynamic_lagrangian: u_stride=%lld", (long long)a->u_stride);
  for (int k = 0; k < a->gdim; ++k)
    if (a->periodic[k] && (!std::isfinite(a->lo[k]) || !std::isfinite(a->hi[k]) || !(a->period[k] > 0.0) ||
                           !std::isfinite(a->period[k]) || !(a->hi[k] > a->lo[k])))
      OX_FAIL("ox_dynamic_lagrangian: periodic axis %d with box %g .. %g, period %g", k, a->lo[k], a->hi[k], a->period[k]);
  if (a->n_vertices == 0) return 0;
  if (a->n_cells < 1 || a->n_cells > (int64_t)0x7fffffff) OX_FAIL("ox_dynamic_lagrangian: n_cells=%lld", (long long)a->n_cells);
  if (!a->x || !a->u || !a->hint || !a->cell_inv || !a->cell_verts || !a->src || !a->delta)
    OX_FAIL("ox_dynamic_lagrangian: null argument (x, u, hint, cell_inv, cell_verts, src, delta)");
  if (!a->f_old || !a->f_new || !a->cs2v || !a->status) OX_FAIL("ox_dynamic_lagrangian: null argument (f_old, f_new, cs2v, status)");
  if (a->f_old == a->f_new) OX_FAIL("ox_dynamic_lagrangian: f_new is f_old; lanes read their neighbours' old values");
  TracerParams P;
  memset(&P, 0, sizeof(P));
  P.G = L->grid;
  P.n_loc = L->n_cells, P.n_bins = L->n_bins, P.n_list = L->n_list;
  P.bin_ptr = L->bin_ptr, P.list = L->list, P.x0 = L->x0, P.grad = L->grad;
  P.tol = a->tol, P.use_hint = 1;
  LagParams A;
  memset(&A, 0, sizeof(A));
  A.n = a->n_vertices, A.x = a->x, A.u = a->u, A.u_stride = a->u_stride, A.hint = a->hint;
  A.cell_inv = a->cell_inv, A.n_cells = a->n_cells, A.cell_verts = a->cell_verts;
  A.src = a->src, A.delta = a->delta, A.f_old = a->f_old, A.f_new = a->f_new, A.cs2v = a->cs2v, A.status = a->status;
  A.h = a->h, A.time_scale = a->time_scale, A.cs2_floor = a->cs2_floor, A.cs2_max = a->cs2_max;
  A.cs2_initial = a->cs2_initial, A.first = a->first ? 1 : 0;
  for (int k = 0; k < a->gdim; ++k)
    A.periodic[k] = a->periodic[k] ? 1 : 0, A.lo[k] = a->lo[k], A.hi[k] = a->hi[k], A.period[k] = a->period[k];
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((a->n_vertices + 255) / 256)), blk(256);
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_LAGRANGIAN, st, a->n_vertices);
  if (a->gdim == 2) hipLaunchKernelGGL((k_dyn_lagrangian<2>), grid, blk, 0, st, P, A);
  else hipLaunchKernelGGL((k_dyn_lagrangian<3>), grid, blk, 0, st, P, A);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Distance to the nearest wall facet.  The locator's grid over the bounding box of the facets
// (segments in 2-D, triangles in 3-D), per bin the ascending list of the facets whose box overlaps it.  A query takes one
// lane per point: the bin of the point (clamped into the grid: points outside are legal), then rings of bins of growing
// Chebyshev radius r around it.  Kept: (d2, position), ties to the lower position -- a minimum that does not depend on the
// order of the visits.  After ring r a facet that was not met lies, on some axis, wholly in bins below b - r or above
// b + r: it is at least min_k min(x_k - edge(b_k - r), edge(b_k + r + 1) - x_k) away (sides that leave the grid do not
// count), less a rounding allowance; the walk stops when d2 <= that bound squared, or when the rings cover the grid.
// The per-facet distance forms the closest point q and d2 = |x - q|^2 from the difference vector: exact zeros on the
// vertices, an error of eps L elsewhere.  It is a pure function of (x, facet), so (dist, nearest) are the same bits
// whatever the grid.  No atomics, no LDS, no scratch.
struct ox_walldist {
  int gdim;
  int64_t n_f, n_bins, n_list;
  LocGrid grid;
  double h[3];       // bin widths (1 on an axis without extent: one bin, never an edge to measure against)
  void *mem;         // xyz, box
  void *mem_grid;    // bin_ptr
  void *mem_list;
  double *xyz;       // [n_f][D][D] vertices
  double *box;       // [n_f][2 D]
  int64_t *bin_ptr;  // [n_bins + 1]
  int32_t *list;     // [n_list] facet positions, ascending inside every bin
};

struct WdVec {
  double v[3];
};

// boxes of the facets and the block's box and summed extents (k_loc_geom's record for k_loc_box)
template <int D>
__global__ __launch_bounds__(256) void k_wd_geom(int64_t n, const double *__restrict__ xyz, double *__restrict__ box,
                                                 double *__restrict__ partial) {
  double mn[D], mx[D], sm[D];
#pragma unroll
  for (int k = 0; k < D; ++k) mn[k] = INFINITY, mx[k] = -INFINITY, sm[k] = 0.0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double l = xyz[i * D * D + k], h = l;
#pragma unroll
      for (int a = 1; a < D; ++a) l = fmin(l, xyz[(i * D + a) * D + k]), h = fmax(h, xyz[(i * D + a) * D + k]);
      const bool ok = isfinite(l) && isfinite(h);  // (a facet with a non-finite vertex: in no bin, never the nearest)
      box[i * 2 * D + k] = ok ? l : INFINITY, box[i * 2 * D + D + k] = ok ? h : -INFINITY;
      if (ok) mn[k] = l, mx[k] = h, sm[k] = h - l;
    }
  }
  loc_block_box<D>(mn, mx, sm, partial);
}

// squared distance of x to the segment (a, b): the clamped projection
__device__ __forceinline__ double wd_facet_d2(const double *__restrict__ f, const double (&x)[2]) {
  const double a[2] = {f[0], f[1]}, b[2] = {f[2], f[3]};
  const double ab[2] = {b[0] - a[0], b[1] - a[1]}, ap[2] = {x[0] - a[0], x[1] - a[1]};
  const double num = fma(ap[1], ab[1], ap[0] * ab[0]), den = fma(ab[1], ab[1], ab[0] * ab[0]);
  double q[2];
  if (!(num > 0.0)) q[0] = a[0], q[1] = a[1];
  else if (num >= den) q[0] = b[0], q[1] = b[1];
  else {
    const double t = num / den;
    q[0] = fma(t, ab[0], a[0]), q[1] = fma(t, ab[1], a[1]);
  }
  const double d0 = x[0] - q[0], d1 = x[1] - q[1];
  return fma(d1, d1, d0 * d0);
}

__device__ __forceinline__ double wd_dot3(const double (&u)[3], const double (&v)[3]) {
  return fma(u[2], v[2], fma(u[1], v[1], u[0] * v[0]));
}

// squared distance of x to the triangle (a, b, c): the closest point by its seven regions (three vertices, three edges,
// the face)
__device__ __forceinline__ double wd_facet_d2(const double *__restrict__ f, const double (&x)[3]) {
  double a[3], b[3], c[3], ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = f[k], b[k] = f[3 + k], c[k] = f[6 + k];
    ab[k] = b[k] - a[k], ac[k] = c[k] - a[k];
    ap[k] = x[k] - a[k], bp[k] = x[k] - b[k], cp[k] = x[k] - c[k];
  }
  const double d1 = wd_dot3(ab, ap), d2 = wd_dot3(ac, ap), d3 = wd_dot3(ab, bp), d4 = wd_dot3(ac, bp);
  const double d5 = wd_dot3(ab, cp), d6 = wd_dot3(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0 && d2 <= 0.0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = a[k];
  } else if (d3 >= 0.0 && d4 <= d3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = b[k];
  } else if (d6 >= 0.0 && d5 <= d6) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = c[k];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double t = d1 / (d1 - d3);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = fma(t, ab[k], a[k]);
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double t = d2 / (d2 - d6);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = fma(t, ac[k], a[k]);
  } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = fma(t, c[k] - b[k], b[k]);
  } else {
    const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = fma(w, ac[k], fma(v, ab[k], a[k]));
  }
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = x[k] - q[k];
  return wd_dot3(d, d);
}

// the ring walk of a finite point x: (best, best_f) = the squared distance to the nearest facet and its position, ties to
// the lower position; old_d: a distance known already (INFINITY: none) -- the walk may stop once nothing unmet beats it
template <int D>
__device__ __forceinline__ void wd_nearest(const double (&x)[D], const LocGrid &G, const WdVec &H, int64_t n_f, int64_t n_bins,
                                           const int64_t *__restrict__ bin_ptr, const int32_t *__restrict__ list,
                                           int64_t n_list, const double *__restrict__ xyz, double old_d, double &best_out,
                                           int32_t &best_f_out) {
  // b: the point's bin, clamped; slack: what the roundings of loc_bin and of the edges below can move an edge by
  int b0 = 0, b1 = 0, b2 = 0;
  double slack = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const int b = loc_bin(G, k, x[k]);
    if (k == 0) b0 = b;
    else if (k == 1) b1 = b;
    else b2 = b;
    slack = fmax(slack, 1e-14 * (fabs(x[k]) + fabs(G.lo[k]) + fabs(G.hi[k])));
  }
  const int nb0 = G.nb[0], nb1 = G.nb[1], nb2 = G.nb[2];
  double best = INFINITY;
  int32_t best_f = -1;
  auto visit = [&](int64_t bin) {
    if (bin < 0 || bin >= n_bins) return;
    int64_t s0 = bin_ptr[bin], s1 = bin_ptr[bin + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > n_list) s1 = n_list;
    for (int64_t s = s0; s < s1; ++s) {
      const int32_t f = list[s];
      if (f < 0 || (int64_t)f >= n_f) continue;
      const double d2 = wd_facet_d2(xyz + (size_t)f * D * D, x);
      if (d2 < best || (d2 == best && f < best_f)) best = d2, best_f = f;  // (NaN: never)
    }
  };
  const int rmax = max(nb0, max(nb1, nb2));
  for (int r = 0; r < rmax; ++r) {
    const int z0 = max(b2 - r, 0), z1 = min(b2 + r, nb2 - 1), y0 = max(b1 - r, 0), y1 = min(b1 + r, nb1 - 1);
    const int x0 = max(b0 - r, 0), x1 = min(b0 + r, nb0 - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int64_t row = ((int64_t)z * nb1 + y) * nb0;
        if (abs(z - b2) == r || abs(y - b1) == r) {  // a row of the shell's faces: all of it
          for (int xx = x0; xx <= x1; ++xx) visit(row + xx);
        } else {  // the shell's two end bins of the row
          if (b0 - r >= 0) visit(row + b0 - r);
          if (b0 + r < nb0) visit(row + b0 + r);
        }
      }
    if (x0 == 0 && x1 == nb0 - 1 && y0 == 0 && y1 == nb1 - 1 && z0 == 0 && z1 == nb2 - 1) break;  // the whole grid
    // the nearest a facet met in no ring so far can be
    double bound = INFINITY;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const int bk = k == 0 ? b0 : (k == 1 ? b1 : b2), nbk = k == 0 ? nb0 : (k == 1 ? nb1 : nb2);
      if (bk - r > 0) bound = fmin(bound, x[k] - fma((double)(bk - r), H.v[k], G.lo[k]));
      if (bk + r < nbk - 1) bound = fmin(bound, fma((double)(bk + r + 1), H.v[k], G.lo[k]) - x[k]);
    }
    bound -= slack;
    if (bound > 0.0 && (best <= bound * bound || old_d < bound)) break;
  }
  best_out = best, best_f_out = best_f;
}

template <int D>
__global__ __launch_bounds__(256) void k_wd_query(int64_t n, const double *__restrict__ xs, WdVec shift, int merge, LocGrid G,
                                                  WdVec H, int64_t n_f, int64_t n_bins,
                                                  const int64_t *__restrict__ bin_ptr, const int32_t *__restrict__ list,
                                                  int64_t n_list, const double *__restrict__ xyz,
                                                  double *__restrict__ dist, int32_t *__restrict__ nearest) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x[D];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = xs[i * D + k] + shift.v[k];
    finite = finite && isfinite(x[k]);
  }
  if (!finite) {  // touches no table
    dist[i] = NAN, nearest[i] = -1;
    return;
  }
  double old_d = INFINITY;
  int32_t old_f = -1;
  if (merge) {
    old_d = dist[i], old_f = nearest[i];
    if (!(old_d >= 0.0) || old_f < 0) old_d = INFINITY, old_f = -1;  // (nothing kept yet)
  }
  double best;
  int32_t best_f;
  wd_nearest<D>(x, G, H, n_f, n_bins, bin_ptr, list, n_list, xyz, old_d, best, best_f);
  double d = sqrt(best);
  int32_t f = best_f;
  if (best_f < 0) d = NAN;  // (no facet with a finite distance)
  if (old_f >= 0 && (f < 0 || old_d < d || (old_d == d && old_f < f))) d = old_d, f = old_f;
  dist[i] = d, nearest[i] = f;
}

// The particles that left the mesh in this advance (facet == OX_PARTICLE_PENDING; every other lane returns at once): the
// nearest exterior facet of the point that left, by the ring walk above; a facet whose action is 1 deposits the particle
// (status 3, velocity 0).  facet = -1: no facet with a finite distance.
template <int D>
__global__ __launch_bounds__(256) void k_particle_classify(int64_t n, const double *__restrict__ xq, LocGrid G, WdVec H,
                                                           int64_t n_f, int64_t n_bins, const int64_t *__restrict__ bin_ptr,
                                                           const int32_t *__restrict__ list, int64_t n_list,
                                                           const double *__restrict__ xyz, const int32_t *__restrict__ action,
                                                           int32_t *__restrict__ facet, int32_t *__restrict__ status,
                                                           double *__restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (facet[i] != OX_PARTICLE_PENDING) return;
  double x[D];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[k] = xq[i * D + k];
    finite = finite && isfinite(x[k]);
  }
  double best = INFINITY;
  int32_t f = -1;
  if (finite) wd_nearest<D>(x, G, H, n_f, n_bins, bin_ptr, list, n_list, xyz, (double)INFINITY, best, f);
  facet[i] = f;
  if (f >= 0 && (int64_t)f < n_f && action[f] == 1) {
    status[i] = 3;
#pragma unroll
    for (int k = 0; k < D; ++k) v[i * D + k] = 0.0;
  }
}

static void wd_free(ox_walldist *W) {
  if (!W) return;
  if (W->mem) (void)hipFree(W->mem);
  if (W->mem_grid) (void)hipFree(W->mem_grid);
  if (W->mem_list) (void)hipFree(W->mem_list);
  delete W;
}

template <int D>
static int wd_create(ox_walldist *W, const double *facet_xyz, const int *bins3, hipStream_t st) {
  const int64_t n = W->n_f;
  const int nblk = (int)((n + 255) / 256);
  const size_t dbl = (size_t)n * (D * D + 2 * D) + (size_t)nblk * 3 * D + 3 * D;
  if (hipMalloc(&W->mem, dbl * sizeof(double)) != hipSuccess)
    OX_FAIL("ox_walldist_create: hipMalloc of %zu bytes failed", dbl * sizeof(double));
  double *p = static_cast<double *>(W->mem);
  W->xyz = p, p += (size_t)n * D * D;
  W->box = p, p += (size_t)n * 2 * D;
  double *partial = p;
  p += (size_t)nblk * 3 * D;
  double *gbox = p;
  OX_HIP(hipMemcpyAsync(W->xyz, facet_xyz, (size_t)n * D * D * sizeof(double), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_wd_geom<D>, dim3(nblk), dim3(256), 0, st, n, W->xyz, W->box, partial);
  OX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loc_box<D>, dim3(1), dim3(256), 0, st, partial, nblk, gbox);
  OX_LAUNCH_CHECK();
  double hb[3 * D];
  OX_HIP(hipMemcpyAsync(hb, gbox, sizeof(hb), hipMemcpyDeviceToHost, st));
  OX_HIP(hipStreamSynchronize(st));
  if (loc_size_grid<D>("ox_walldist_create", W->grid, hb, n, bins3, &W->n_bins)) return -1;
  for (int k = 0; k < 3; ++k) {
    const double ext = W->grid.hi[k] - W->grid.lo[k];
    W->h[k] = k < D && ext > 0.0 ? ext / (double)W->grid.nb[k] : 1.0;
  }
  return loc_build_lists<D>("ox_walldist_create", W->grid, W->box, n, W->n_bins, st, &W->mem_grid, &W->bin_ptr, &W->mem_list,
                            &W->list, &W->n_list);
}

extern "C" int ox_walldist_create(int gdim, const double *facet_xyz, int64_t n_facets, const int *bins3, void *stream,
                                  ox_walldist **out) {
  if (!out) OX_FAIL("ox_walldist_create: null argument");
  *out = nullptr;
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_walldist_create: gdim=%d", gdim);
  if (!facet_xyz || n_facets < 1) OX_FAIL("ox_walldist_create: no wall facets (n_facets=%lld)", (long long)n_facets);
  if (n_facets >= ((int64_t)1 << 31) - 256) OX_FAIL("ox_walldist_create: %lld facets", (long long)n_facets);
  if (bins3)
    for (int k = 0; k < gdim; ++k)
      if (bins3[k] < 1 || bins3[k] > 1024) OX_FAIL("ox_walldist_create: bins3[%d]=%d (1..1024)", k, bins3[k]);
  ox_walldist *W = new ox_walldist();
  memset(W, 0, sizeof(*W));
  W->gdim = gdim, W->n_f = n_facets;
  hipStream_t st = ox_stream(stream);
  const int rc = gdim == 2 ? wd_create<2>(W, facet_xyz, bins3, st) : wd_create<3>(W, facet_xyz, bins3, st);
  if (rc) {
    wd_free(W);
    return -1;
  }
  *out = W;
  return 0;
}

extern "C" int ox_walldist_destroy(ox_walldist *W) {
  wd_free(W);
  return 0;
}

extern "C" int ox_walldist_info(const ox_walldist *W, int64_t *n_facets, int64_t *n_bins, int64_t *n_list, int *bins_per_axis) {
  if (!W) OX_FAIL("ox_walldist_info: null handle");
  if (n_facets) *n_facets = W->n_f;
  if (n_bins) *n_bins = W->n_bins;
  if (n_list) *n_list = W->n_list;
  if (bins_per_axis)
    for (int k = 0; k < 3; ++k) bins_per_axis[k] = W->grid.nb[k];
  return 0;
}

extern "C" int ox_walldist_query(const ox_walldist *W, int64_t n_points, const double *x, const double *shift, int merge,
                                 double *dist, int32_t *nearest, void *stream) {
  if (!W || (n_points > 0 && (!x || !dist || !nearest))) OX_FAIL("ox_walldist_query: null argument");
  if (n_points <= 0) return 0;
  WdVec s{{0.0, 0.0, 0.0}}, H{{W->h[0], W->h[1], W->h[2]}};
  if (shift)
    for (int k = 0; k < W->gdim; ++k) {
      if (!std::isfinite(shift[k])) OX_FAIL("ox_walldist_query: shift[%d] is not finite", k);
      s.v[k] = shift[k];
    }
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((n_points + 255) / 256));
  if (W->gdim == 2)
    hipLaunchKernelGGL(k_wd_query<2>, grid, dim3(256), 0, st, n_points, x, s, merge ? 1 : 0, W->grid, H, W->n_f, W->n_bins,
                       W->bin_ptr, W->list, W->n_list, W->xyz, dist, nearest);
  else
    hipLaunchKernelGGL(k_wd_query<3>, grid, dim3(256), 0, st, n_points, x, s, merge ? 1 : 0, W->grid, H, W->n_f, W->n_bins,
                       W->bin_ptr, W->list, W->n_list, W->xyz, dist, nearest);
  OX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Inertial particles: the advance (k_particle_advance) and, behind it on the same stream, the classification of the
// particles that left in it (k_particle_classify).
extern "C" int ox_particle_advance(const ox_particle_args *a, void *stream) {
  if (!a) OX_FAIL("ox_particle_advance: null argument (args)");
  if (!a->loc || !a->walls) OX_FAIL("ox_particle_advance: null argument (loc, walls)");
  if (a->gdim != 2 && a->gdim != 3) OX_FAIL("ox_particle_advance: gdim=%d", a->gdim);
  if (a->degree < 1 || a->degree > 3) OX_FAIL("ox_particle_advance: degree %d (1..3)", a->degree);
  if (a->nc < a->gdim || a->nc > OX_MAXC) OX_FAIL("ox_particle_advance: nc=%d (gdim=%d..%d)", a->nc, a->gdim, OX_MAXC);
  if (a->substeps < 1 || a->substeps > OX_TRACER_MAX_SUBSTEPS)
    OX_FAIL("ox_particle_advance: substeps=%d (1..%d)", a->substeps, OX_TRACER_MAX_SUBSTEPS);
  if (a->scheme != OX_PARTICLE_EXP1 && a->scheme != OX_PARTICLE_EXP2) OX_FAIL("ox_particle_advance: scheme=%d", a->scheme);
  if (a->drag != OX_PARTICLE_STOKES && a->drag != OX_PARTICLE_SCHILLER_NAUMANN) OX_FAIL("ox_particle_advance: drag=%d", a->drag);
  if (!std::isfinite(a->dt) || !std::isfinite(a->t)) OX_FAIL("ox_particle_advance: dt=%g at t=%g is not finite", a->dt, a->t);
  if (!std::isfinite(a->nu) || a->nu < 0.0) OX_FAIL("ox_particle_advance: nu=%g (finite, >= 0)", a->nu);
  if (a->drag == OX_PARTICLE_SCHILLER_NAUMANN && !(a->nu > 0.0))
    OX_FAIL("ox_particle_advance: the Schiller-Naumann law needs nu > 0 (nu=%g)", a->nu);
  for (int k = 0; k < a->gdim; ++k) {
    if (!std::isfinite(a->g[k])) OX_FAIL("ox_particle_advance: g[%d] is not finite", k);
    if (a->periodic[k] && (!std::isfinite(a->lo[k]) || !std::isfinite(a->hi[k]) || !(a->period[k] > 0.0) ||
                           !std::isfinite(a->period[k]) || !(a->hi[k] > a->lo[k])))
      OX_FAIL("ox_particle_advance: periodic axis %d with box %g .. %g, period %g", k, a->lo[k], a->hi[k], a->period[k]);
  }
  const ox_locator *L = a->loc;
  const ox_walldist *W = a->walls;
  if (L->ids) OX_FAIL("ox_particle_advance: a locator over a selection of cells; particles take the whole-mesh locator");
  if (L->gdim != a->gdim || W->gdim != a->gdim)
    OX_FAIL("ox_particle_advance: loc->gdim=%d, walls->gdim=%d, gdim=%d", L->gdim, W->gdim, a->gdim);
  if (a->n_mesh_cells != L->n_cells)
    OX_FAIL("ox_particle_advance: n_mesh_cells=%lld, the locator holds %lld", (long long)a->n_mesh_cells, (long long)L->n_cells);
  if (a->n_facets != W->n_f)
    OX_FAIL("ox_particle_advance: n_facets=%lld, the wall structure holds %lld", (long long)a->n_facets, (long long)W->n_f);
  if (!(a->tol >= 0.0) || a->tol > L->tol) OX_FAIL("ox_particle_advance: tol=%g, the grid was built for tol <= %g", a->tol, L->tol);
  if (a->n < 0) OX_FAIL("ox_particle_advance: n=%lld", (long long)a->n);
  if (a->n == 0) return 0;
  if (!a->cell_dofs || !a->cell_inv || !a->u_a || !a->u_b || a->n_cells < 1 || a->n_rows < 1)
    OX_FAIL("ox_particle_advance: null argument (cell_dofs, cell_inv, u_a, u_b)");
  if (!a->x || !a->v || !a->cell || !a->status || !a->age || !a->path || !a->t_exit)
    OX_FAIL("ox_particle_advance: null argument (x, v, cell, status, age, path, t_exit)");
  if (!a->wraps || !a->facet || !a->xq || !a->tau_p || !a->diam || !a->beta || !a->facet_action)
    OX_FAIL("ox_particle_advance: null argument (wraps, facet, xq, tau_p, diam, beta, facet_action)");
  TracerParams P;
  P.G = L->grid;
  P.n_loc = L->n_cells, P.n_bins = L->n_bins, P.n_list = L->n_list;
  P.bin_ptr = L->bin_ptr, P.list = L->list, P.x0 = L->x0, P.grad = L->grad;
  P.cell_dofs = a->cell_dofs, P.n_cells = a->n_cells, P.n_rows = a->n_rows, P.cell_inv = a->cell_inv;
  P.u_a = a->u_a, P.u_b = a->u_b, P.nc = a->nc;
  P.t = a->t, P.dt = a->dt, P.tol = a->tol;
  P.substeps = a->substeps, P.scheme = a->scheme, P.use_hint = a->use_hint ? 1 : 0;
  P.n = a->n, P.x = a->x, P.cell = a->cell, P.status = a->status, P.age = a->age, P.path = a->path, P.t_exit = a->t_exit;
  ParticleParams A;
  memset(&A, 0, sizeof(A));
  A.v = a->v, A.wraps = a->wraps, A.facet = a->facet, A.xq = a->xq;
  A.tau_p = a->tau_p, A.diam = a->diam, A.beta = a->beta;
  A.nu = a->nu, A.drag = a->drag;
  for (int k = 0; k < a->gdim; ++k) {
    A.g[k] = a->g[k];
    A.periodic[k] = a->periodic[k] ? 1 : 0, A.lo[k] = a->lo[k], A.hi[k] = a->hi[k], A.period[k] = a->period[k];
  }
  hipStream_t st = ox_stream(stream);
  const dim3 grid((unsigned)((a->n + 255) / 256)), blk(256);
  switch (a->gdim * 10 + a->degree) {
    case 21: hipLaunchKernelGGL((k_particle_advance<2, 1>), grid, blk, 0, st, P, A); break;
    case 22: hipLaunchKernelGGL((k_particle_advance<2, 2>), grid, blk, 0, st, P, A); break;
    case 23: hipLaunchKernelGGL((k_particle_advance<2, 3>), grid, blk, 0, st, P, A); break;
    case 31: hipLaunchKernelGGL((k_particle_advance<3, 1>), grid, blk, 0, st, P, A); break;
    case 32: hipLaunchKernelGGL((k_particle_advance<3, 2>), grid, blk, 0, st, P, A); break;
    default: hipLaunchKernelGGL((k_particle_advance<3, 3>), grid, blk, 0, st, P, A); break;
  }
  OX_LAUNCH_CHECK();
  const WdVec H{{W->h[0], W->h[1], W->h[2]}};
  if (a->gdim == 2)
    hipLaunchKernelGGL(k_particle_classify<2>, grid, blk, 0, st, a->n, a->xq, W->grid, H, W->n_f, W->n_bins, W->bin_ptr, W->list,
                       W->n_list, W->xyz, a->facet_action, a->facet, a->status, a->v);
  else
    hipLaunchKernelGGL(k_particle_classify<3>, grid, blk, 0, st, a->n, a->xq, W->grid, H, W->n_f, W->n_bins, W->bin_ptr, W->list,
                       W->n_list, W->xyz, a->facet_action, a->facet, a->status, a->v);
  OX_LAUNCH_CHECK();
  return 0;
}
