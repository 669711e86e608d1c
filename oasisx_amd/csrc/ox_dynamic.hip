// The dynamic Smagorinsky model: the Germano-Lilly procedure on a simplicial mesh.
//
// Per cell c (kernel cell order), from u_ab as the nut kernel (ox_viscosity.hip) reads it: u_c, g_c at the centroid,
// S_c = sym g_c, s_c = sqrt(2 S_c:S_c), D_c = |c|^(2/gdim), |c| = |det J| / gdim!.  The test filter of a per-cell
// quantity q is the vertex-patch top hat
//   q_v  = sum_{c in patch(v)} |c| q_c / sum_{c in patch(v)} |c|       (cells in ascending kernel cell id)
//   q^_c = (1/(gdim+1)) sum_a q_{v_a(c)}                               (local vertex order)
// over vertex CLASSES (a periodic mesh's patches wrap around the seam).  With r = filter_ratio
//   L = (u u^T)^ - u^ u^^T,  Ld = L - (tr L / gdim) I,  M = r^2 D_c |S^| S^ - (D s S)^,  |S^| = sqrt(2 S^:S^)
//   LM_c = Ld:M,  MM_c = M:M,  Cs2 = -(1/2) <LM> / <MM>,  clipped to [0, cs2_max], 0 where <MM> is not positive
// and nut_c = Cs2_c D_c s_c.  <.> is a volume-weighted sum over the cells of a bin (one bin: the global average) or the
// test filter applied once more (the local average).
//
// Launches (all one lane per cell / vertex / one block per chunk, no atomics, no LDS beyond the block sum, every sum
// in ONE order -- two launches on equal inputs give equal bits):
//   ox_dynamic_cells      rec[c]  = {u_c (GD), S_c upper triangle row by row (NS), D_c s_c, |c|}      NR = GD + NS + 2
//   ox_dynamic_vertices   mom[v]  = {u, u u^T (NS), S (NS), D s S (NS)} filtered to the vertex        NM = GD + 3 NS
//   ox_dynamic_products   lm[c]   = {LM_c, MM_c}
//   ox_dynamic_bin_sums / ox_dynamic_bin_coefficients   the chunk plan of ProfileStatistics: partial sums per chunk,
//                         then one wave per bin: bins[b] = {sum |c| LM, sum |c| MM, Cs2 unclipped, Cs2 clipped}
//   ox_patch_filter_vertices / ox_patch_filter_cells    the test filter of K = 1, 2 fields (the local average; PatchFilter)
//   ox_dynamic_clip       cs2[c]  = clip(-(1/2) a_c / b_c) of a pair field
// and then ox_cell_viscosity with the table of Cs2 (ox_viscosity.hip): nut_c = Cs2 D_c s_c, Cs2 read per cell or through
// the cell's bin.
// The vertex pass is lane-per-vertex: a patch holds at most a few tens of cells (24 on the Kuhn lattice), every lane keeps
// its NM running sums in registers and adds its cells in ascending order; a sub-wave per vertex would need a cross-lane
// sum of NM values per vertex and another summation order.
#include "fe_tables_cv.h"
#include "ox_element.h"
#include <cmath>

namespace {

__host__ __device__ constexpr int dyn_ns(int gdim) { return gdim * (gdim + 1) / 2; }
__host__ __device__ constexpr int dyn_nr(int gdim) { return gdim + dyn_ns(gdim) + 2; }
__host__ __device__ constexpr int dyn_nm(int gdim) { return gdim + 3 * dyn_ns(gdim); }
static_assert(dyn_nr(2) == 7 && dyn_nr(3) == 11 && dyn_nm(2) == 11 && dyn_nm(3) == 21, "record and moment sizes");

template <int GDIM, int DEG>
__host__ __device__ constexpr const auto &ox_phic() {
  OX_FE_PICK(GDIM, DEG, OX_PHIC, );
}

__device__ __forceinline__ double dyn_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// -(1/2) lm / mm clipped to [0, cmax]; 0 where mm is not positive; a NaN in either stays a NaN
__device__ __forceinline__ double dyn_ratio(double lm, double mm) { return -0.5 * lm / mm; }
__device__ __forceinline__ double dyn_clip(double lm, double mm, double cmax) {
  if (mm > 0.0) {
    const double c = dyn_ratio(lm, mm);
    return c < 0.0 ? 0.0 : (c > cmax ? cmax : c);  // (NaN fails both comparisons)
  }
  return (mm != mm || lm != lm) ? dyn_nan() : 0.0;
}

// A:B of two symmetric tensors given by their upper triangles (row by row): diagonal once, the rest twice
template <int GDIM>
__device__ __forceinline__ double dyn_sym_dot(const double (&a)[dyn_ns(GDIM)], const double (&b)[dyn_ns(GDIM)]) {
  double s = 0.0;
  int m = 0;
#pragma unroll
  for (int i = 0; i < GDIM; ++i)
#pragma unroll
    for (int j = i; j < GDIM; ++j, ++m) s = fma(i == j ? a[m] : 2.0 * a[m], b[m], s);
  return s;
}

// ---- 1. the cell pass: the centroid prologue of the nut kernel (ox_element.h), plus u at the centroid
template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_dyn_cells(ox_cells cells, const int32_t *__restrict__ cell_dofs,
                                                   const double *__restrict__ uab, double *__restrict__ rec) {
  constexpr int ND = ox_nd(GDIM, DEG), NS = dyn_ns(GDIM), NR = dyn_nr(GDIM);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cells.n_cells) return;
  double uc[ND][GDIM], g[GDIM][GDIM], adet;
  ox_centroid_grad<GDIM, DEG>(cells, cell_dofs, uab, e, g, uc, adet);
  const double ss = ox_sym_sq<GDIM>(g);
  const double vol = ox_cell_volume<GDIM>(adet);
  double *__restrict__ r = rec + (size_t)e * NR;
#pragma unroll
  for (int d = 0; d < GDIM; ++d) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < ND; ++i)
      if (ox_phic<GDIM, DEG>()[i] != 0.0) v = fma(uc[i][d], ox_phic<GDIM, DEG>()[i], v);
    r[d] = v;
  }
  int m = 0;
#pragma unroll
  for (int i = 0; i < GDIM; ++i)
#pragma unroll
    for (int j = i; j < GDIM; ++j, ++m) r[GDIM + m] = 0.5 * (g[i][j] + g[j][i]);
  r[GDIM + NS] = ox_delta2_of_volume<GDIM>(vol) * sqrt(2.0 * ss);
  r[GDIM + NS + 1] = vol;
}

// ---- 2. the vertex pass: one lane per vertex class, its cells in ascending order
template <int GDIM>
__global__ __launch_bounds__(256) void k_dyn_vertices(int64_t n_vertices, const int32_t *__restrict__ ptr,
                                                      const int32_t *__restrict__ idx, int64_t n_cells,
                                                      const double *__restrict__ rec, double *__restrict__ mom) {
  constexpr int NS = dyn_ns(GDIM), NR = dyn_nr(GDIM), NM = dyn_nm(GDIM);
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_vertices) return;
  const int p0 = ptr[v], p1 = ptr[v + 1];
  double a[NM], w = 0.0;
  bool bad = p0 < 0 || p1 <= p0 || (int64_t)p1 > n_cells * (GDIM + 1);
#pragma unroll
  for (int i = 0; i < NM; ++i) a[i] = 0.0;
  if (!bad)
    for (int p = p0; p < p1; ++p) {
      const int32_t c = idx[p];
      if (c < 0 || (int64_t)c >= n_cells) {
        bad = true;
        break;
      }
      const double *__restrict__ r = rec + (size_t)c * NR;
      double q[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) q[i] = r[i];
      const double vol = q[NR - 1], ds = q[NR - 2];
      w += vol;
#pragma unroll
      for (int d = 0; d < GDIM; ++d) a[d] = fma(vol, q[d], a[d]);
      int m = 0;
#pragma unroll
      for (int i = 0; i < GDIM; ++i)
#pragma unroll
        for (int j = i; j < GDIM; ++j, ++m) {
          a[GDIM + m] = fma(vol, q[i] * q[j], a[GDIM + m]);
          a[GDIM + NS + m] = fma(vol, q[GDIM + m], a[GDIM + NS + m]);
          a[GDIM + 2 * NS + m] = fma(vol, ds * q[GDIM + m], a[GDIM + 2 * NS + m]);
        }
    }
  double *__restrict__ o = mom + (size_t)v * NM;
  const double inv = 1.0 / w;
#pragma unroll
  for (int i = 0; i < NM; ++i) o[i] = bad ? dyn_nan() : a[i] * inv;
}

// q^ of NQ consecutive doubles per vertex at the GDIM + 1 vertices of cell e; false where a vertex is out of range
template <int GDIM, int NQ>
__device__ __forceinline__ bool dyn_cell_mean(const int32_t *__restrict__ cell_verts, int64_t e, int64_t n_vertices,
                                              const double *__restrict__ qv, double (&f)[NQ]) {
  int32_t vv[GDIM + 1];
  bool ok = true;
#pragma unroll
  for (int a = 0; a <= GDIM; ++a) {
    vv[a] = cell_verts[(size_t)e * (GDIM + 1) + a];
    ok = ok && vv[a] >= 0 && (int64_t)vv[a] < n_vertices;
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) f[i] = 0.0;
  if (!ok) return false;
#pragma unroll
  for (int a = 0; a <= GDIM; ++a) {
    const double *__restrict__ p = qv + (size_t)vv[a] * NQ;
#pragma unroll
    for (int i = 0; i < NQ; ++i) f[i] += p[i];
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) f[i] *= 1.0 / (GDIM + 1);
  return true;
}

// ---- 3. the product pass
template <int GDIM>
__global__ __launch_bounds__(256) void k_dyn_products(int64_t n_cells, const int32_t *__restrict__ cell_verts,
                                                      int64_t n_vertices, const double *__restrict__ rec,
                                                      const double *__restrict__ mom, double r2, double *__restrict__ lm) {
  constexpr int NS = dyn_ns(GDIM), NR = dyn_nr(GDIM), NM = dyn_nm(GDIM);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_cells) return;
  double f[NM];
  if (!dyn_cell_mean<GDIM, NM>(cell_verts, e, n_vertices, mom, f)) {
    lm[2 * e] = lm[2 * e + 1] = dyn_nan();
    return;
  }
  const double d2 = ox_delta2_of_volume<GDIM>(rec[(size_t)e * NR + NR - 1]);
  double L[NS], S[NS], M[NS];
  int m = 0;
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < GDIM; ++i)
#pragma unroll
    for (int j = i; j < GDIM; ++j, ++m) {
      L[m] = fma(-f[i], f[j], f[GDIM + m]);
      S[m] = f[GDIM + NS + m];
      if (i == j) tr += L[m];
    }
  tr *= 1.0 / GDIM;
  m = 0;
#pragma unroll
  for (int i = 0; i < GDIM; ++i)
#pragma unroll
    for (int j = i; j < GDIM; ++j, ++m)
      if (i == j) L[m] -= tr;
  const double c = r2 * d2 * sqrt(2.0 * dyn_sym_dot<GDIM>(S, S));
#pragma unroll
  for (int k = 0; k < NS; ++k) M[k] = fma(c, S[k], -f[GDIM + 2 * NS + k]);
  lm[2 * e] = dyn_sym_dot<GDIM>(L, M);
  lm[2 * e + 1] = dyn_sym_dot<GDIM>(M, M);
}

// ---- 4a. bins: one block per chunk of the plan (chunk = {first entry of order, cells, bin, consecutive})
__global__ __launch_bounds__(256) void k_dyn_bin_sums(int64_t n_cells, const double *__restrict__ lm,
                                                      const double *__restrict__ vol, int64_t vol_stride,
                                                      const int32_t *__restrict__ order, const int4 *__restrict__ chunk,
                                                      double *__restrict__ partials) {
  __shared__ double lds[4 * 2];
  const int4 ch = chunk[blockIdx.x];
  const int len = ch.y < 256 ? ch.y : 256;
  double v[2] = {0.0, 0.0};
  int64_t e = -1;
  if ((int)threadIdx.x < len) e = ch.w ? (int64_t)order[ch.x] + threadIdx.x : (int64_t)order[(int64_t)ch.x + threadIdx.x];
  if (e >= 0 && e < n_cells) {
    const double w = vol[(size_t)e * vol_stride];
    v[0] = w * lm[2 * e];
    v[1] = w * lm[2 * e + 1];
  }
  ox_block_sum_256<2>(v, lds);
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = v[0];
    partials[2 * (size_t)blockIdx.x + 1] = v[1];
  }
}

// one wave per bin: the bin's chunk rows lane-strided in ascending order, a wave sum, the ratio and its clip
__global__ __launch_bounds__(64) void k_dyn_bin_coef(const int32_t *__restrict__ bin_chunk_ptr,
                                                     const double *__restrict__ partials, double cmax,
                                                     double *__restrict__ bins) {
  const int64_t bin = blockIdx.x;
  const int c0 = bin_chunk_ptr[bin], c1 = bin_chunk_ptr[bin + 1];
  double a = 0.0, b = 0.0;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 64) {
    a += partials[2 * (size_t)c];
    b += partials[2 * (size_t)c + 1];
  }
  a = ox_wave_sum(a);
  b = ox_wave_sum(b);
  if (threadIdx.x != 0) return;
  double *__restrict__ o = bins + 4 * (size_t)bin;
  o[0] = a;
  o[1] = b;
  o[2] = dyn_ratio(a, b);
  o[3] = dyn_clip(a, b, cmax);
}

// ---- 4b. the test filter of K fields given per cell
template <int K>
__global__ __launch_bounds__(256) void k_filter_vertices(int64_t n_vertices, const int32_t *__restrict__ ptr,
                                                         const int32_t *__restrict__ idx, int64_t n_cells, int64_t n_idx,
                                                         const double *__restrict__ q, const double *__restrict__ vol,
                                                         int64_t vol_stride, double *__restrict__ qv) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n_vertices) return;
  const int p0 = ptr[v], p1 = ptr[v + 1];
  double a[K], w = 0.0;
  bool bad = p0 < 0 || p1 <= p0 || (int64_t)p1 > n_idx;
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = 0.0;
  if (!bad)
    for (int p = p0; p < p1; ++p) {
      const int32_t c = idx[p];
      if (c < 0 || (int64_t)c >= n_cells) {
        bad = true;
        break;
      }
      const double wc = vol[(size_t)c * vol_stride];
      w += wc;
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] = fma(wc, q[(size_t)c * K + k], a[k]);
    }
  const double inv = 1.0 / w;
#pragma unroll
  for (int k = 0; k < K; ++k) qv[(size_t)v * K + k] = bad ? dyn_nan() : a[k] * inv;
}

template <int GDIM, int K>
__global__ __launch_bounds__(256) void k_filter_cells(int64_t n_cells, const int32_t *__restrict__ cell_verts,
                                                      int64_t n_vertices, const double *__restrict__ qv,
                                                      double *__restrict__ qf) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_cells) return;
  double f[K];
  const bool ok = dyn_cell_mean<GDIM, K>(cell_verts, e, n_vertices, qv, f);
#pragma unroll
  for (int k = 0; k < K; ++k) qf[(size_t)e * K + k] = ok ? f[k] : dyn_nan();
}

__global__ __launch_bounds__(256) void k_dyn_clip(int64_t n, const double *__restrict__ pairs, double cmax,
                                                  double *__restrict__ cs2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  cs2[e] = dyn_clip(pairs[2 * e], pairs[2 * e + 1], cmax);
}

static inline int64_t dyn_blocks(int64_t n) { return (n + 255) / 256; }

}  // namespace

#define OX_DYN_COUNT(who, what, n)                                                     \
  if ((n) <= 0 || (n) > (int64_t)0x7fffffff) OX_FAIL(who ": " what "=%lld", (long long)(n))

extern "C" int ox_dynamic_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab, double *rec,
                                void *stream) {
  if (!cells || !cell_dofs || !uab || !rec || !cells->geom) OX_FAIL("ox_dynamic_cells: null argument");
  const int64_t nblk = ox_cell_blocks("ox_dynamic_cells", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
#define OX_DYN_CASE(GD, DG)                                                                                         \
  if (g == GD && degree == DG) {                                                                                    \
    if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_CELLS, st, cells->n_cells);                                        \
    hipLaunchKernelGGL((k_dyn_cells<GD, DG>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, uab, rec);           \
    if (ox_prof_on) ox_prof_stop(st);                                                                               \
    OX_LAUNCH_CHECK();                                                                                              \
    return 0;                                                                                                       \
  }
  OX_FOR_GDIM_DEG(OX_DYN_CASE)
#undef OX_DYN_CASE
  OX_FAIL("ox_dynamic_cells: unsupported gdim=%d degree=%d", g, degree);
}

extern "C" int ox_dynamic_vertices(int gdim, int64_t n_vertices, const int32_t *ptr, const int32_t *idx, int64_t n_cells,
                                   const double *rec, double *mom, void *stream) {
  if (!ptr || !idx || !rec || !mom) OX_FAIL("ox_dynamic_vertices: null argument");
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_dynamic_vertices: gdim=%d", gdim);
  OX_DYN_COUNT("ox_dynamic_vertices", "n_vertices", n_vertices);
  OX_DYN_COUNT("ox_dynamic_vertices", "n_cells", n_cells);
  OX_DYN_COUNT("ox_dynamic_vertices", "n_cells x (gdim + 1)", n_cells * (gdim + 1));
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_VERTICES, st, n_vertices);
  if (gdim == 2)
    hipLaunchKernelGGL((k_dyn_vertices<2>), dim3(dyn_blocks(n_vertices)), dim3(256), 0, st, n_vertices, ptr, idx, n_cells,
                       rec, mom);
  else
    hipLaunchKernelGGL((k_dyn_vertices<3>), dim3(dyn_blocks(n_vertices)), dim3(256), 0, st, n_vertices, ptr, idx, n_cells,
                       rec, mom);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_dynamic_products(int gdim, int64_t n_cells, const int32_t *cell_verts, int64_t n_vertices,
                                   const double *rec, const double *mom, double filter_ratio, double *lm, void *stream) {
  if (!cell_verts || !rec || !mom || !lm) OX_FAIL("ox_dynamic_products: null argument");
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_dynamic_products: gdim=%d", gdim);
  if (!(filter_ratio > 1.0) || !std::isfinite(filter_ratio)) OX_FAIL("ox_dynamic_products: filter_ratio=%g", filter_ratio);
  OX_DYN_COUNT("ox_dynamic_products", "n_vertices", n_vertices);
  OX_DYN_COUNT("ox_dynamic_products", "n_cells", n_cells);
  hipStream_t st = ox_stream(stream);
  const double r2 = filter_ratio * filter_ratio;
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_PRODUCTS, st, n_cells);
  if (gdim == 2)
    hipLaunchKernelGGL((k_dyn_products<2>), dim3(dyn_blocks(n_cells)), dim3(256), 0, st, n_cells, cell_verts, n_vertices,
                       rec, mom, r2, lm);
  else
    hipLaunchKernelGGL((k_dyn_products<3>), dim3(dyn_blocks(n_cells)), dim3(256), 0, st, n_cells, cell_verts, n_vertices,
                       rec, mom, r2, lm);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_dynamic_bin_sums(int64_t n_cells, const double *lm, const double *vol, int64_t vol_stride,
                                   const int32_t *order, const int32_t *chunks, int64_t n_chunks, double *partials,
                                   void *stream) {
  if (!lm || !vol || !order || !chunks || !partials) OX_FAIL("ox_dynamic_bin_sums: null argument");
  OX_DYN_COUNT("ox_dynamic_bin_sums", "n_cells", n_cells);
  OX_DYN_COUNT("ox_dynamic_bin_sums", "n_chunks", n_chunks);
  if (vol_stride < 1) OX_FAIL("ox_dynamic_bin_sums: vol_stride=%lld", (long long)vol_stride);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_BIN_SUMS, st, n_chunks);
  hipLaunchKernelGGL(k_dyn_bin_sums, dim3((unsigned)n_chunks), dim3(256), 0, st, n_cells, lm, vol, vol_stride, order,
                     reinterpret_cast<const int4 *>(chunks), partials);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_dynamic_bin_coefficients(int64_t n_bins, const int32_t *bin_chunk_ptr, const double *partials,
                                           double cs2_max, double *bins, void *stream) {
  if (!bin_chunk_ptr || !partials || !bins) OX_FAIL("ox_dynamic_bin_coefficients: null argument");
  OX_DYN_COUNT("ox_dynamic_bin_coefficients", "n_bins", n_bins);
  if (!(cs2_max >= 0.0) || !std::isfinite(cs2_max)) OX_FAIL("ox_dynamic_bin_coefficients: cs2_max=%g", cs2_max);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_BIN_COEF, st, n_bins);
  hipLaunchKernelGGL(k_dyn_bin_coef, dim3((unsigned)n_bins), dim3(64), 0, st, bin_chunk_ptr, partials, cs2_max, bins);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_patch_filter_vertices(int k, int64_t n_vertices, const int32_t *ptr, const int32_t *idx, int64_t n_cells,
                                        int64_t n_idx, const double *q, const double *vol, int64_t vol_stride, double *qv,
                                        void *stream) {
  if (!ptr || !idx || !q || !vol || !qv) OX_FAIL("ox_patch_filter_vertices: null argument");
  if (k != 1 && k != 2) OX_FAIL("ox_patch_filter_vertices: k=%d (1 and 2 are instantiated)", k);
  OX_DYN_COUNT("ox_patch_filter_vertices", "n_vertices", n_vertices);
  OX_DYN_COUNT("ox_patch_filter_vertices", "n_cells", n_cells);
  OX_DYN_COUNT("ox_patch_filter_vertices", "n_idx", n_idx);
  if (vol_stride < 1) OX_FAIL("ox_patch_filter_vertices: vol_stride=%lld", (long long)vol_stride);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_PATCH_FILTER, st, n_vertices);
  if (k == 1)
    hipLaunchKernelGGL((k_filter_vertices<1>), dim3(dyn_blocks(n_vertices)), dim3(256), 0, st, n_vertices, ptr, idx, n_cells,
                       n_idx, q, vol, vol_stride, qv);
  else
    hipLaunchKernelGGL((k_filter_vertices<2>), dim3(dyn_blocks(n_vertices)), dim3(256), 0, st, n_vertices, ptr, idx, n_cells,
                       n_idx, q, vol, vol_stride, qv);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_patch_filter_cells(int k, int gdim, int64_t n_cells, const int32_t *cell_verts, int64_t n_vertices,
                                     const double *qv, double *qf, void *stream) {
  if (!cell_verts || !qv || !qf) OX_FAIL("ox_patch_filter_cells: null argument");
  if (k != 1 && k != 2) OX_FAIL("ox_patch_filter_cells: k=%d (1 and 2 are instantiated)", k);
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_patch_filter_cells: gdim=%d", gdim);
  OX_DYN_COUNT("ox_patch_filter_cells", "n_vertices", n_vertices);
  OX_DYN_COUNT("ox_patch_filter_cells", "n_cells", n_cells);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_PATCH_FILTER, st, n_cells);
#define OX_FILT_CASE(GD, K_)                                                                                       \
  if (gdim == GD && k == K_)                                                                                       \
    hipLaunchKernelGGL((k_filter_cells<GD, K_>), dim3(dyn_blocks(n_cells)), dim3(256), 0, st, n_cells, cell_verts, \
                       n_vertices, qv, qf);
  OX_FILT_CASE(2, 1) OX_FILT_CASE(2, 2) OX_FILT_CASE(3, 1) OX_FILT_CASE(3, 2)
#undef OX_FILT_CASE
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

extern "C" int ox_dynamic_clip(int64_t n, const double *pairs, double cs2_max, double *cs2, void *stream) {
  if (!pairs || !cs2) OX_FAIL("ox_dynamic_clip: null argument");
  OX_DYN_COUNT("ox_dynamic_clip", "n", n);
  if (!(cs2_max >= 0.0) || !std::isfinite(cs2_max)) OX_FAIL("ox_dynamic_clip: cs2_max=%g", cs2_max);
  hipStream_t st = ox_stream(stream);
  if (ox_prof_on) ox_prof_start(OX_TAG_DYNAMIC_BIN_COEF, st, n);
  hipLaunchKernelGGL(k_dyn_clip, dim3(dyn_blocks(n)), dim3(256), 0, st, n, pairs, cs2_max, cs2);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}
