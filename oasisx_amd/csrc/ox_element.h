// The element prologue shared by the per-cell and per-facet kernels: dof and geometry-record
// sizes, the choice of a generated table by (GDIM, DEG), a cell's dof / geometry / coefficient loads, the gradient
// contraction and the facet normal.  Every sum has ONE order, written here: the kernels that call these agree bit for bit.
#pragma once
#include "fe_tables_c.h"
#include "fe_tables_f.h"
#include "fe_tables_o.h"
#include "ox_kernels.h"
#include <cmath>
#include <type_traits>

// dofs of the Lagrange element of degree 1, 2, 3 on a simplex, and doubles of a cell's geometry record
// (GDIM rows grad lambda_1..GDIM, |det J|, padding)
__host__ __device__ constexpr int ox_nd(int gdim, int deg) {
  return deg == 1 ? gdim + 1 : (deg == 3 ? (gdim == 2 ? 10 : 20) : (gdim == 2 ? 6 : 10));
}
__host__ __device__ constexpr int ox_gs(int gdim) { return gdim == 2 ? 6 : 10; }
static_assert(ox_nd(2, 1) == 3 && ox_nd(2, 2) == 6 && ox_nd(2, 3) == 10, "P1, P2, P3 triangles");
static_assert(ox_nd(3, 1) == 4 && ox_nd(3, 2) == 10 && ox_nd(3, 3) == 20, "P1, P2, P3 tetrahedra");

// The body of a function that returns STEM<GDIM>_<DEG> IDX of the generated tables, e.g.
// OX_FE_PICK(GDIM, DEG, OX_DPHIC, [i][b]); an empty IDX returns the table itself.
#define OX_FE_PICK(GDIM, DEG, STEM, IDX)                                                                 \
  static_assert((GDIM == 2 || GDIM == 3) && DEG >= 1 && DEG <= 3, "simplices, Lagrange degree 1, 2, 3"); \
  if constexpr (GDIM == 2 && DEG == 1) return STEM##2_1 IDX;                                             \
  else if constexpr (GDIM == 2 && DEG == 2) return STEM##2_2 IDX;                                        \
  else if constexpr (GDIM == 2) return STEM##2_3 IDX;                                                    \
  else if constexpr (DEG == 1) return STEM##3_1 IDX;                                                     \
  else if constexpr (DEG == 2) return STEM##3_2 IDX;                                                     \
  else return STEM##3_3 IDX

// dphi_i/dlambda_b at the centroid [i][b], its facet means [a][i][b] and the facet means of the basis [a][i]
// (compile-time constants)
template <int GDIM, int DEG>
__host__ __device__ constexpr const auto &ox_dphic() {
  OX_FE_PICK(GDIM, DEG, OX_DPHIC, );
}
template <int GDIM, int DEG>
__host__ __device__ constexpr const auto &ox_dphif() {
  OX_FE_PICK(GDIM, DEG, OX_DPHIF, );
}
template <int GDIM, int DEG>
__host__ __device__ constexpr const auto &ox_phif() {
  OX_FE_PICK(GDIM, DEG, OX_PHIF, );
}

template <int ND>
__device__ __forceinline__ void ox_load_dofs(const int32_t *__restrict__ cell_dofs, int64_t e, int32_t (&dd)[ND]) {
#pragma unroll
  for (int i = 0; i < ND; ++i) dd[i] = cell_dofs[(size_t)e * ND + i];
}

// uc[i][c] = u[dd[i] * NC + c]: NC = GDIM for a velocity, 1 for a pressure
template <int ND, int NC>
__device__ __forceinline__ void ox_gather(const int32_t (&dd)[ND], const double *__restrict__ u, double (&uc)[ND][NC]) {
#pragma unroll
  for (int i = 0; i < ND; ++i)
#pragma unroll
    for (int c = 0; c < NC; ++c) uc[i][c] = u[(size_t)dd[i] * NC + c];
}

// G[b] = grad lambda_b (G[0] = -sum of the others) and |det J| from a cell's geometry record
template <int GDIM>
__device__ __forceinline__ double ox_geom_adet(const double *__restrict__ gp) {
  return gp[GDIM * GDIM];
}
template <int GDIM>
__device__ __forceinline__ void ox_load_geom(const double *__restrict__ gp, double (&G)[GDIM + 1][GDIM], double &adet) {
#pragma unroll
  for (int d = 0; d < GDIM; ++d) G[0][d] = 0.0;
#pragma unroll
  for (int a = 1; a <= GDIM; ++a)
#pragma unroll
    for (int d = 0; d < GDIM; ++d) {
      G[a][d] = gp[(a - 1) * GDIM + d];
      G[0][d] -= G[a][d];
    }
  adet = ox_geom_adet<GDIM>(gp);
}

// t[d][b] += sum_i uc[i][d] tab[i][b] in dof order; tab is a compile-time table, its zero entries cost nothing
template <int GDIM, int ND>
__device__ __forceinline__ void ox_contract(const double (&uc)[ND][GDIM], const double (&tab)[ND][GDIM + 1],
                                            double (&t)[GDIM][GDIM + 1]) {
#pragma unroll
  for (int i = 0; i < ND; ++i)
#pragma unroll
    for (int b = 0; b <= GDIM; ++b)
      if (tab[i][b] != 0.0) {
#pragma unroll
        for (int d = 0; d < GDIM; ++d) t[d][b] = fma(uc[i][d], tab[i][b], t[d][b]);
      }
}

// g[d][k] = sum_{b >= b0} t[d][b] G[b][k]
template <int GDIM>
__device__ __forceinline__ void ox_grad_from_t(const double (&t)[GDIM][GDIM + 1], const double (&G)[GDIM + 1][GDIM],
                                               double (&g)[GDIM][GDIM], int b0 = 0) {
#pragma unroll
  for (int d = 0; d < GDIM; ++d)
#pragma unroll
    for (int k = 0; k < GDIM; ++k) {
      double v = 0.0;
#pragma unroll
      for (int b = 0; b <= GDIM; ++b)
        if (b >= b0) v = fma(t[d][b], G[b][k], v);
      g[d][k] = v;
    }
}

// S:S, S = (g + g^T)/2
template <int GDIM>
__device__ __forceinline__ double ox_sym_sq(const double (&g)[GDIM][GDIM]) {
  double ss = 0.0;
#pragma unroll
  for (int d = 0; d < GDIM; ++d)
#pragma unroll
    for (int k = 0; k < GDIM; ++k) {
      const double s = 0.5 * (g[d][k] + g[k][d]);
      ss = fma(s, s, ss);
    }
  return ss;
}

// The centroid prologue of the nut kernel and ox_dynamic_cells: round 1 the cell's dofs and geometry (both indexed by e),
// round 2 the coefficient gathers; uc[i][d] = u_ab at the cell's dofs, g[d][k] = d(u_ab)_d / dx_k, adet = |det J|
template <int GDIM, int DEG>
__device__ __forceinline__ void ox_centroid_grad(const ox_cells &cells, const int32_t *__restrict__ cell_dofs,
                                                 const double *__restrict__ uab, int64_t e, double (&g)[GDIM][GDIM],
                                                 double (&uc)[ox_nd(GDIM, DEG)][GDIM], double &adet) {
  constexpr int ND = ox_nd(GDIM, DEG);
  int32_t dd[ND];
  ox_load_dofs<ND>(cell_dofs, e, dd);
  double G[GDIM + 1][GDIM];
  ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
  ox_gather<ND, GDIM>(dd, uab, uc);
  double t[GDIM][GDIM + 1] = {};
  ox_contract<GDIM, ND>(uc, ox_dphic<GDIM, DEG>(), t);
  ox_grad_from_t<GDIM>(t, G, g);
}

// |cell| = |det J| / gdim! and Delta^2 = |cell|^(2/gdim), from the volume or from |det J|
template <int GDIM>
__device__ __forceinline__ double ox_cell_volume(double adet) { return GDIM == 2 ? 0.5 * adet : adet * (1.0 / 6.0); }
template <int GDIM>
__device__ __forceinline__ double ox_delta2_of_volume(double vol) {
  if constexpr (GDIM == 2) return vol;
  const double h = cbrt(vol);
  return h * h;
}
template <int GDIM>
__device__ __forceinline__ double ox_delta2(double adet) { return ox_delta2_of_volume<GDIM>(ox_cell_volume<GDIM>(adet)); }

// The facet opposite local vertex a, Ga = grad lambda_a: outward unit normal n = -Ga / |Ga| and measure
// |det J| |Ga| / (GDIM - 1)!
template <int GDIM>
__device__ __forceinline__ void ox_facet_normal(const double (&Ga)[GDIM], double adet, double (&n)[GDIM], double &area) {
  double ga2 = 0.0;
#pragma unroll
  for (int d = 0; d < GDIM; ++d) ga2 = fma(Ga[d], Ga[d], ga2);
  const double ga = sqrt(ga2);
#pragma unroll
  for (int d = 0; d < GDIM; ++d) n[d] = -Ga[d] / ga;
  area = adet * ga * (GDIM == 3 ? 0.5 : 1.0);
}

// The facet rule of the backflow term and of the scalars' flux / Robin conditions: its size and tables, indexed at run
// time (constant memory).  The facet basis at the rule's points is the same on every local facet (facet dofs and points
// both in ascending local vertex order).
template <int GDIM, int DU>
struct ox_facet_rule {
  static constexpr int NP = DU == 1 ? 2 : (DU == 2 ? 4 : 5);
  static constexpr int NQ = GDIM == 2 ? NP : NP * NP;
  static constexpr int NFD = GDIM == 2 ? DU + 1 : (DU + 1) * (DU + 2) / 2;
  __device__ static double w(int q) { OX_FE_PICK(GDIM, DU, OX_OW, [q]); }
  __device__ static double phi(int q, int j) { OX_FE_PICK(GDIM, DU, OX_OPHI, [q][j]); }
  __device__ static int fd(int a, int j) { OX_FE_PICK(GDIM, DU, OX_OFD, [a][j]); }
};

// outward unit normal and measure of local facet a (0 <= a <= GDIM) from the cell's geometry record: the one row
// grad lambda_a is selected as the rows are read, no G[GDIM + 1][GDIM] is kept
template <int GDIM>
__device__ __forceinline__ void ox_facet_geometry(const double *__restrict__ gp, int a, double (&n)[GDIM], double &area) {
  double Ga[GDIM];
#pragma unroll
  for (int d = 0; d < GDIM; ++d) {
    double g0 = 0.0, ga = 0.0;
#pragma unroll
    for (int b = 1; b <= GDIM; ++b) {
      const double g = gp[(b - 1) * GDIM + d];
      g0 -= g;
      if (b == a) ga = g;
    }
    Ga[d] = a == 0 ? g0 : ga;
  }
  ox_facet_normal<GDIM>(Ga, ox_geom_adet<GDIM>(gp), n, area);
}

// f(std::integral_constant<int, a>) for the run-time local facet 0 <= a <= GDIM: one instantiation of f per facet
template <int GDIM, class F>
__device__ __forceinline__ void ox_facet_dispatch(int a, F &&f) {
  if (a == 0) f(std::integral_constant<int, 0>{});
  else if (a == 1) f(std::integral_constant<int, 1>{});
  else if (a == 2) f(std::integral_constant<int, 2>{});
  else if constexpr (GDIM == 3) f(std::integral_constant<int, 3>{});
}

// ---- host side: M(gdim, degree, further arguments...) for the six elements
#define OX_FOR_GDIM_DEG(M, ...)                                         \
  M(2, 1, ##__VA_ARGS__) M(2, 2, ##__VA_ARGS__) M(2, 3, ##__VA_ARGS__) \
  M(3, 1, ##__VA_ARGS__) M(3, 2, ##__VA_ARGS__) M(3, 3, ##__VA_ARGS__)

// 256-lane blocks of a launch with one lane per cell: 0 for an empty mesh, -1 with "<who>: <n> cells" as the error
// beyond INT32_MAX cells
static inline int64_t ox_cell_blocks(const char *who, const ox_cells *cells) {
  if (cells->n_cells <= 0) return 0;
  if (cells->n_cells > (int64_t)0x7fffffff) {
    snprintf(ox_err_buf, sizeof(ox_err_buf), "%s: %lld cells", who, (long long)cells->n_cells);
    return -1;
  }
  return (cells->n_cells + 255) / 256;
}
