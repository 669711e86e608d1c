// Eddy viscosity per cell: nut[e] from grad u_ab at the cell's centroid, for the fused
// assemble_first with a per-cell viscosity (ox_assemble_first with ox_first_args.nut).
//
//   g[d][k] = d(u_ab)_d / dx_k = sum_i u_ab[dof_i][d] sum_b dphi_i/dlambda_b (centroid) G[b][k]
//   S       = (g + g^T)/2,   Delta^2 = |cell|^(2/gdim),  |cell| = |det J| / gdim!
//   Smagorinsky:  nut = Cs^2 Delta^2 sqrt(2 S:S)
//   WALE (3-D):   Sd  = sym(g g) - tr(g g)/3 I,  x = Sd:Sd,  y = S:S
//                 nut = Cw^2 Delta^2 x sqrt(x) / (y^2 sqrt(y) + x sqrt(sqrt(x))),  0 where the denominator is 0
//
// Generalised-Newtonian laws, gd = sqrt(2 S:S), nut = max(nu(gd) - base, 0):
//   Carreau-Yasuda:  nu = nu_inf + (nu0 - nu_inf) (1 + (lam gd)^a)^((n - 1)/a),  base = min(nu0, nu_inf)
//   Cross:           nu = nu_inf + (nu0 - nu_inf) / (1 + (lam gd)^m),            base = min(nu0, nu_inf)
//   power law:       nu = min(max(k gd^(n - 1), nu_min), nu_max),                base = nu_min
//                    (gd == 0: nu_max for n < 1, nu_min for n > 1, the clipped k for n == 1 -- no 0^negative)
//
// One lane per cell, in kernel cell order: the cell's dof list (ND x 4 B) and geometry record (GS x 8 B) are streamed,
// the ND x GDIM coefficients are gathered, 8 B are written.  The centroid derivatives are compile-time constants
// (fe_tables_c.h): identically-zero entries cost nothing.  No atomics, no LDS; every sum has a fixed order.
#include "ox_element.h"
#include <cmath>

namespace {

#define OX_NUT_SMAGORINSKY 0
#define OX_NUT_WALE 1
#define OX_NUT_CARREAU_YASUDA 2
#define OX_NUT_CROSS 3
#define OX_NUT_POWER_LAW 4

// The parameters of a generalised-Newtonian law, by value in the kernel arguments (the eddy-viscosity models keep their
// one double).  Carreau-Yasuda: c0 = nu_inf, c1 = nu0 - nu_inf, c2 = lam, c3 = a, c4 = (n - 1)/a;  Cross: c0 = nu_inf,
// c1 = nu0 - nu_inf, c2 = lam, c3 = m;  power law: c0 = k, c1 = n - 1, c2 = nu_min, c3 = nu_max.
struct LawParams {
  double c0, c1, c2, c3, c4, base;
};
template <int MODEL>
using NutArg = std::conditional_t<(MODEL >= OX_NUT_CARREAU_YASUDA), LawParams, double>;

// van Driest damping: the tables of ox_vandriest by value; nothing where the flag is off
struct NoDamping {};
template <int VD>
using DampArg = std::conditional_t<(VD != 0), ox_vandriest, NoDamping>;

template <int GDIM, int DEG, int MODEL, int VD = 0>
__global__ __launch_bounds__(256) void k_eddy_viscosity(ox_cells cells, const int32_t *__restrict__ cell_dofs,
                                                        const double *__restrict__ uab, NutArg<MODEL> coef2,
                                                        double *__restrict__ nut, DampArg<VD> vd) {
  constexpr int ND = ox_nd(GDIM, DEG);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cells.n_cells) return;
  // round 1: the cell's dofs and geometry (both indexed by e); round 2: the coefficient gathers
  int32_t dd[ND];
  ox_load_dofs<ND>(cell_dofs, e, dd);
  double G[GDIM + 1][GDIM], adet;
  ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
  double uc[ND][GDIM];
  ox_gather<ND, GDIM>(dd, uab, uc);
  double t[GDIM][GDIM + 1] = {}, g[GDIM][GDIM];
  ox_contract<GDIM, ND>(uc, ox_dphic<GDIM, DEG>(), t);
  ox_grad_from_t<GDIM>(t, G, g);
  const double ss = ox_sym_sq<GDIM>(g);
  // Delta^2 = |cell|^(2/gdim)
  double delta2;
  if constexpr (GDIM == 2) delta2 = 0.5 * adet;
  else {
    const double h = cbrt(adet * (1.0 / 6.0));
    delta2 = h * h;
  }
  double out;
  if constexpr (MODEL == OX_NUT_SMAGORINSKY && VD != 0) {
    // D = 1 - exp(-y+ / A+), y+ = d u_tau / nu, u_tau = sqrt(|wss|) of the centroid's nearest wall facet
    const int32_t f = vd.nearest[e];
    if (f < 0 || (int64_t)f >= vd.n_facets) {
      out = __longlong_as_double(0x7ff8000000000000LL);
    } else {
      double ut = vd.u_tau;
      if (vd.wss) {
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < GDIM; ++k) {
          const double w = vd.wss[(size_t)f * GDIM + k];
          m2 = fma(w, w, m2);
        }
        ut = sqrt(sqrt(m2));
      }
      const double yp = vd.dist[e] * ut / vd.nu;
      const double dmp = -expm1(-yp / vd.a_plus);
      out = coef2 * delta2 * (dmp * dmp) * sqrt(2.0 * ss);
    }
  } else if constexpr (MODEL == OX_NUT_SMAGORINSKY) {
    out = coef2 * delta2 * sqrt(2.0 * ss);
  } else if constexpr (MODEL == OX_NUT_CARREAU_YASUDA) {
    const double gd = sqrt(2.0 * ss);
    const double nu = fma(coef2.c1, pow(1.0 + pow(coef2.c2 * gd, coef2.c3), coef2.c4), coef2.c0);
    out = fmax(nu - coef2.base, 0.0);
  } else if constexpr (MODEL == OX_NUT_CROSS) {
    const double gd = sqrt(2.0 * ss);
    const double nu = coef2.c0 + coef2.c1 / (1.0 + pow(coef2.c2 * gd, coef2.c3));
    out = fmax(nu - coef2.base, 0.0);
  } else if constexpr (MODEL == OX_NUT_POWER_LAW) {
    const double gd = sqrt(2.0 * ss);
    double nu;
    if (gd > 0.0) nu = coef2.c0 * pow(gd, coef2.c1);
    else nu = coef2.c1 < 0.0 ? coef2.c3 : (coef2.c1 > 0.0 ? coef2.c2 : coef2.c0);
    nu = fmin(fmax(nu, coef2.c2), coef2.c3);
    out = fmax(nu - coef2.base, 0.0);
  } else {
    static_assert(GDIM == 3, "WALE is built for three dimensions");
    double g2[GDIM][GDIM];
#pragma unroll
    for (int d = 0; d < GDIM; ++d)
#pragma unroll
      for (int k = 0; k < GDIM; ++k) {
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < GDIM; ++m) v = fma(g[d][m], g[m][k], v);
        g2[d][k] = v;
      }
    const double tr3 = (g2[0][0] + g2[1][1] + g2[2][2]) * (1.0 / 3.0);
    double x = 0.0;  // Sd:Sd
#pragma unroll
    for (int d = 0; d < GDIM; ++d)
#pragma unroll
      for (int k = 0; k < GDIM; ++k) {
        const double s = 0.5 * (g2[d][k] + g2[k][d]) - (d == k ? tr3 : 0.0);
        x = fma(s, s, x);
      }
    const double num = x * sqrt(x);
    const double den = ss * ss * sqrt(ss) + x * sqrt(sqrt(x));
    out = den > 0.0 ? coef2 * delta2 * (num / den) : 0.0;
  }
  nut[e] = out;
}

}  // namespace

extern "C" int ox_eddy_viscosity(int model, int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab,
                                 double coefficient, double *nut, void *stream) {
  if (!cells || !cell_dofs || !uab || !nut || !cells->geom) OX_FAIL("ox_eddy_viscosity: null argument");
  if (!(coefficient >= 0.0)) OX_FAIL("ox_eddy_viscosity: coefficient=%g", coefficient);
  const int64_t nblk = ox_cell_blocks("ox_eddy_viscosity", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const double c2 = coefficient * coefficient;
  if (model == OX_NUT_WALE && g != 3) OX_FAIL("ox_eddy_viscosity: WALE is built for gdim = 3 (got %d)", g);
  if (model != OX_NUT_SMAGORINSKY && model != OX_NUT_WALE) OX_FAIL("ox_eddy_viscosity: model=%d", model);
#define OX_NUT_CASE(GD, DG, MD)                                                                                        \
  if (g == GD && degree == DG && model == MD) {                                                                        \
    if (ox_prof_on) ox_prof_start(OX_TAG_EDDY_VISCOSITY, st, cells->n_cells);                                          \
    hipLaunchKernelGGL((k_eddy_viscosity<GD, DG, MD>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, uab, c2, nut, \
                       NoDamping{});                                                                                   \
    if (ox_prof_on) ox_prof_stop(st);                                                                                  \
    OX_LAUNCH_CHECK();                                                                                                 \
    return 0;                                                                                                          \
  }
  OX_FOR_GDIM_DEG(OX_NUT_CASE, OX_NUT_SMAGORINSKY)
  OX_NUT_CASE(3, 1, OX_NUT_WALE) OX_NUT_CASE(3, 2, OX_NUT_WALE) OX_NUT_CASE(3, 3, OX_NUT_WALE)
#undef OX_NUT_CASE
  OX_FAIL("ox_eddy_viscosity: unsupported gdim=%d degree=%d", g, degree);
}

// Smagorinsky with van Driest damping: k_eddy_viscosity with the damping flag; 12 B more per cell are streamed (dist,
// nearest) and gdim doubles of wss gathered.
extern "C" int ox_eddy_viscosity_damped(int model, int degree, const ox_cells *cells, const int32_t *cell_dofs,
                                        const double *uab, double coefficient, const ox_vandriest *vd, double *nut,
                                        void *stream) {
  if (!cells || !cell_dofs || !uab || !nut || !cells->geom || !vd) OX_FAIL("ox_eddy_viscosity_damped: null argument");
  if (!vd->dist || !vd->nearest) OX_FAIL("ox_eddy_viscosity_damped: null argument (dist, nearest)");
  if (!(coefficient >= 0.0)) OX_FAIL("ox_eddy_viscosity_damped: coefficient=%g", coefficient);
  if (model != OX_NUT_SMAGORINSKY) OX_FAIL("ox_eddy_viscosity_damped: model=%d (0: Smagorinsky)", model);
  if (!(vd->nu > 0.0) || !std::isfinite(vd->nu)) OX_FAIL("ox_eddy_viscosity_damped: nu=%g", vd->nu);
  if (!(vd->a_plus > 0.0) || !std::isfinite(vd->a_plus)) OX_FAIL("ox_eddy_viscosity_damped: a_plus=%g", vd->a_plus);
  if (!vd->wss && (!(vd->u_tau >= 0.0) || !std::isfinite(vd->u_tau))) OX_FAIL("ox_eddy_viscosity_damped: u_tau=%g", vd->u_tau);
  if (vd->n_facets < 1 || vd->n_facets > (int64_t)0x7fffffff)
    OX_FAIL("ox_eddy_viscosity_damped: n_facets=%lld", (long long)vd->n_facets);
  const int64_t nblk = ox_cell_blocks("ox_eddy_viscosity_damped", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const double c2 = coefficient * coefficient;
#define OX_NUT_VD_CASE(GD, DG)                                                                                        \
  if (g == GD && degree == DG) {                                                                                      \
    if (ox_prof_on) ox_prof_start(OX_TAG_EDDY_VISCOSITY, st, cells->n_cells);                                         \
    hipLaunchKernelGGL((k_eddy_viscosity<GD, DG, OX_NUT_SMAGORINSKY, 1>), dim3(nblk), dim3(256), 0, st, *cells,       \
                       cell_dofs, uab, c2, nut, *vd);                                                                 \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_NUT_VD_CASE)
#undef OX_NUT_VD_CASE
  OX_FAIL("ox_eddy_viscosity_damped: unsupported gdim=%d degree=%d", g, degree);
}

// nut[e] = max(nu(gd_e) - base, 0) of a generalised-Newtonian law (include/oasisx_hip.h): the centroid gradient of
// k_eddy_viscosity, the law as one more branch of it.
extern "C" int ox_viscosity_law(int law, int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab,
                                const double *params, int n_params, double *nut, void *stream) {
  if (!cells || !cell_dofs || !uab || !params || !nut || !cells->geom) OX_FAIL("ox_viscosity_law: null argument");
  const int want = law == OX_NUT_CARREAU_YASUDA ? 5 : ((law == OX_NUT_CROSS || law == OX_NUT_POWER_LAW) ? 4 : -1);
  if (want < 0) OX_FAIL("ox_viscosity_law: law=%d (2: Carreau-Yasuda, 3: Cross, 4: power law)", law);
  if (n_params != want) OX_FAIL("ox_viscosity_law: law %d takes %d parameters (got %d)", law, want, n_params);
  for (int k = 0; k < n_params; ++k)
    if (!std::isfinite(params[k])) OX_FAIL("ox_viscosity_law: parameter %d is not finite", k);
  LawParams P{};
  if (law == OX_NUT_POWER_LAW) {
    const double k = params[0], n = params[1], nu_min = params[2], nu_max = params[3];
    if (k < 0.0 || n <= 0.0 || nu_min <= 0.0 || nu_min > nu_max)
      OX_FAIL("ox_viscosity_law: power law k=%g n=%g nu_min=%g nu_max=%g", k, n, nu_min, nu_max);
    P.c0 = k, P.c1 = n - 1.0, P.c2 = nu_min, P.c3 = nu_max, P.base = nu_min;
  } else {
    const double nu0 = params[0], nu_inf = params[1], lam = params[2], e = params[3];
    if (nu0 < 0.0 || nu_inf < 0.0 || lam < 0.0 || e <= 0.0)
      OX_FAIL("ox_viscosity_law: law %d nu0=%g nu_inf=%g lam=%g exponent=%g", law, nu0, nu_inf, lam, e);
    P.c0 = nu_inf, P.c1 = nu0 - nu_inf, P.c2 = lam, P.base = nu0 < nu_inf ? nu0 : nu_inf;
    if (law == OX_NUT_CARREAU_YASUDA) {
      const double a = params[4];
      if (a <= 0.0) OX_FAIL("ox_viscosity_law: Carreau-Yasuda a=%g", a);
      P.c3 = a, P.c4 = (e - 1.0) / a;
    } else {
      P.c3 = e;
    }
  }
  const int64_t nblk = ox_cell_blocks("ox_viscosity_law", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
#define OX_LAW_CASE(GD, DG, MD)                                                                                       \
  if (g == GD && degree == DG && law == MD) {                                                                         \
    if (ox_prof_on) ox_prof_start(OX_TAG_EDDY_VISCOSITY, st, cells->n_cells);                                         \
    hipLaunchKernelGGL((k_eddy_viscosity<GD, DG, MD>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, uab, P, nut, \
                       NoDamping{});                                                                                  \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_LAW_CASE, OX_NUT_CARREAU_YASUDA)
  OX_FOR_GDIM_DEG(OX_LAW_CASE, OX_NUT_CROSS)
  OX_FOR_GDIM_DEG(OX_LAW_CASE, OX_NUT_POWER_LAW)
#undef OX_LAW_CASE
  OX_FAIL("ox_viscosity_law: unsupported gdim=%d degree=%d", g, degree);
}
