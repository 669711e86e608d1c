// Viscosity per cell (DESIGN.md sections 14, 16, 24, 26, 28): nut[e] from grad u_ab at the cell's centroid for
// ox_assemble_first with ox_first_args.nut.  ONE kernel template, ONE entry point; the forms differ in one factor.
//
//   g[d][k] = d(u_ab)_d / dx_k = sum_i u_ab[dof_i][d] sum_b dphi_i/dlambda_b (centroid) G[b][k]
//   S       = (g + g^T)/2,   Delta^2 = |cell|^(2/gdim),  |cell| = |det J| / gdim!
//   Smagorinsky:  nut = C Delta^2 sqrt(2 S:S),  C = Cs^2 | Cs^2 D^2 (van Driest) | cs2[k] (a table, per cell or per bin)
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
// the ND x GDIM coefficients are gathered, 8 B are written (damped: 12 B more streamed, dist and nearest, and gdim doubles
// of wss gathered; table: 8 or 12 B more).  The centroid derivatives are compile-time constants (fe_tables_c.h):
// identically-zero entries cost nothing.  No atomics, no LDS; every sum has a fixed order.
#include "ox_element.h"
#include <cmath>

namespace {

#define OX_NUT_SMAGORINSKY 0
#define OX_NUT_WALE 1
#define OX_NUT_CARREAU_YASUDA 2
#define OX_NUT_CROSS 3
#define OX_NUT_POWER_LAW 4

// FORM, where the Smagorinsky factor comes from: Cs^2 alone, Cs^2 with van Driest damping, a table of Cs2
#define OX_NUT_PLAIN 0
#define OX_NUT_DAMPED 1
#define OX_NUT_TABLE 2

// A law's parameters, by value in the kernel arguments.  Carreau-Yasuda: c0 = nu_inf, c1 = nu0 - nu_inf, c2 = lam, c3 = a,
// c4 = (n - 1)/a;  Cross: the same c0, c1, c2 and c3 = m;  power law: c0 = k, c1 = n - 1, c2 = nu_min, c3 = nu_max.
struct LawParams {
  double c0, c1, c2, c3, c4, base;
};
// Cs2 per cell (cell_bin NULL) or per bin: C = cs2[k stride], k = cell_bin[e] or e
struct CoefTable {
  const double *cs2;
  int64_t stride, n_coef;
  const int32_t *cell_bin;
};
// the model's factor by value: the laws' parameters, the table, or one double (the squared constant)
template <int MODEL, int FORM>
using NutArg = std::conditional_t<(MODEL >= OX_NUT_CARREAU_YASUDA), LawParams,
                                  std::conditional_t<FORM == OX_NUT_TABLE, CoefTable, double>>;

// van Driest damping: the tables of ox_vandriest by value; nothing in the other forms
struct NoDamping {};
template <int FORM>
using DampArg = std::conditional_t<FORM == OX_NUT_DAMPED, ox_vandriest, NoDamping>;

__device__ __forceinline__ double nut_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

template <int GDIM, int DEG, int MODEL, int FORM>
__global__ __launch_bounds__(256) void k_cell_viscosity(ox_cells cells, const int32_t *__restrict__ cell_dofs,
                                                        const double *__restrict__ uab, NutArg<MODEL, FORM> coef2,
                                                        double *__restrict__ nut, DampArg<FORM> vd) {
  static_assert(FORM == OX_NUT_PLAIN || MODEL == OX_NUT_SMAGORINSKY, "damping and the table belong to Smagorinsky");
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cells.n_cells) return;
  double uc[ox_nd(GDIM, DEG)][GDIM], g[GDIM][GDIM], adet;
  ox_centroid_grad<GDIM, DEG>(cells, cell_dofs, uab, e, g, uc, adet);
  const double ss = ox_sym_sq<GDIM>(g);
  const double delta2 = ox_delta2<GDIM>(adet);
  double out;
  if constexpr (FORM == OX_NUT_DAMPED) {
    // D = 1 - exp(-y+ / A+), y+ = d u_tau / nu, u_tau = sqrt(|wss|) of the centroid's nearest wall facet
    const int32_t f = vd.nearest[e];
    if (f < 0 || (int64_t)f >= vd.n_facets) {
      out = nut_nan();
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
  } else if constexpr (FORM == OX_NUT_TABLE) {
    const int64_t k = coef2.cell_bin ? (int64_t)coef2.cell_bin[e] : e;
    double c;
    if (k < 0) c = 0.0;  // a cell outside every bin
    else if (k >= coef2.n_coef) c = nut_nan();
    else c = coef2.cs2[(size_t)k * coef2.stride];
    out = c * delta2 * sqrt(2.0 * ss);
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

// the table form keeps its own profiling tag: recorded profiles stay comparable
template <int GD, int DG, int MODEL, int FORM>
int nut_launch(const ox_cells *cells, const ox_viscosity_args *a, NutArg<MODEL, FORM> coef2, DampArg<FORM> vd, int64_t nblk,
               hipStream_t st) {
  if (ox_prof_on)
    ox_prof_start(FORM == OX_NUT_TABLE ? OX_TAG_EDDY_VISCOSITY_CELLCOEF : OX_TAG_EDDY_VISCOSITY, st, cells->n_cells);
  hipLaunchKernelGGL((k_cell_viscosity<GD, DG, MODEL, FORM>), dim3(nblk), dim3(256), 0, st, *cells, a->cell_dofs, a->uab,
                     coef2, a->nut, vd);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

// the 39 instantiations: per element Smagorinsky plain, damped and from a table, the three laws, and WALE in 3-D
template <int GD, int DG>
int nut_model(const ox_cells *cells, const ox_viscosity_args *a, double c2, const LawParams &P, int64_t nblk,
              hipStream_t st) {
  switch (a->model) {
  case OX_NUT_SMAGORINSKY:
    if (a->cs2)
      return nut_launch<GD, DG, OX_NUT_SMAGORINSKY, OX_NUT_TABLE>(
          cells, a, CoefTable{a->cs2, a->cs2_stride, a->n_coef, a->cell_bin}, {}, nblk, st);
    if (a->damping) return nut_launch<GD, DG, OX_NUT_SMAGORINSKY, OX_NUT_DAMPED>(cells, a, c2, *a->damping, nblk, st);
    return nut_launch<GD, DG, OX_NUT_SMAGORINSKY, OX_NUT_PLAIN>(cells, a, c2, {}, nblk, st);
  case OX_NUT_WALE:
    if constexpr (GD == 3) return nut_launch<GD, DG, OX_NUT_WALE, OX_NUT_PLAIN>(cells, a, c2, {}, nblk, st);
    else OX_FAIL("ox_cell_viscosity: model 1, WALE, is built for gdim = 3 (got %d)", GD);
  case OX_NUT_CARREAU_YASUDA:
    return nut_launch<GD, DG, OX_NUT_CARREAU_YASUDA, OX_NUT_PLAIN>(cells, a, P, {}, nblk, st);
  case OX_NUT_CROSS:
    return nut_launch<GD, DG, OX_NUT_CROSS, OX_NUT_PLAIN>(cells, a, P, {}, nblk, st);
  default:
    return nut_launch<GD, DG, OX_NUT_POWER_LAW, OX_NUT_PLAIN>(cells, a, P, {}, nblk, st);
  }
}

// Every check on the argument block, on the host and before any device call; the laws' parameters end up in P.  A field
// the chosen form does not read must be NULL or 0: a block filled for another form is refused, not half-used.
int nut_check(const ox_cells *cells, const ox_viscosity_args *a, LawParams &P) {
  if (!cells || !a) OX_FAIL("ox_cell_viscosity: null argument (cells, args)");
  if (!cells->geom || !a->cell_dofs || !a->uab || !a->nut) OX_FAIL("ox_cell_viscosity: null geom, cell_dofs, uab or nut");
  const int model = a->model;
  if (model < OX_NUT_SMAGORINSKY || model > OX_NUT_POWER_LAW)
    OX_FAIL("ox_cell_viscosity: model=%d (0: Smagorinsky, 1: WALE, 2: Carreau-Yasuda, 3: Cross, 4: power law)", model);
  if (a->degree < 1 || a->degree > 3) OX_FAIL("ox_cell_viscosity: degree=%d (1, 2, 3)", a->degree);
  const bool law = model >= OX_NUT_CARREAU_YASUDA, table = a->cs2 != nullptr;
  if (!law && (a->params || a->n_params))
    OX_FAIL("ox_cell_viscosity: params, n_params=%d belong to the laws (models 2-4), model=%d", a->n_params, model);
  if ((law || table) && a->coefficient != 0.0)
    OX_FAIL("ox_cell_viscosity: coefficient=%g belongs to models 0 and 1 without cs2 (model=%d)", a->coefficient, model);
  if (model != OX_NUT_SMAGORINSKY && (a->damping || table))
    OX_FAIL("ox_cell_viscosity: damping and cs2 belong to model 0 (model=%d)", model);
  if (table && a->damping) OX_FAIL("ox_cell_viscosity: damping together with cs2 is not instantiated");
  if (!table && (a->cs2_stride || a->n_coef || a->cell_bin))
    OX_FAIL("ox_cell_viscosity: cs2_stride=%lld, n_coef=%lld, cell_bin without cs2", (long long)a->cs2_stride,
            (long long)a->n_coef);
  if (law) {
    const double *params = a->params;
    if (!params) OX_FAIL("ox_cell_viscosity: null argument (params)");
    const int want = model == OX_NUT_CARREAU_YASUDA ? 5 : 4;
    if (a->n_params != want)
      OX_FAIL("ox_cell_viscosity: model %d takes n_params=%d parameters (got %d)", model, want, a->n_params);
    for (int k = 0; k < want; ++k)
      if (!std::isfinite(params[k])) OX_FAIL("ox_cell_viscosity: params[%d] is not finite", k);
    if (model == OX_NUT_POWER_LAW) {
      const double k = params[0], n = params[1], nu_min = params[2], nu_max = params[3];
      if (k < 0.0 || n <= 0.0 || nu_min <= 0.0 || nu_min > nu_max)
        OX_FAIL("ox_cell_viscosity: params of the power law k=%g n=%g nu_min=%g nu_max=%g", k, n, nu_min, nu_max);
      P.c0 = k, P.c1 = n - 1.0, P.c2 = nu_min, P.c3 = nu_max, P.base = nu_min;
    } else {
      const double nu0 = params[0], nu_inf = params[1], lam = params[2], e = params[3];
      if (nu0 < 0.0 || nu_inf < 0.0 || lam < 0.0 || e <= 0.0)
        OX_FAIL("ox_cell_viscosity: params of model %d nu0=%g nu_inf=%g lam=%g exponent=%g", model, nu0, nu_inf, lam, e);
      P.c0 = nu_inf, P.c1 = nu0 - nu_inf, P.c2 = lam, P.base = nu0 < nu_inf ? nu0 : nu_inf;
      if (model == OX_NUT_CARREAU_YASUDA) {
        const double y = params[4];
        if (y <= 0.0) OX_FAIL("ox_cell_viscosity: params of Carreau-Yasuda a=%g", y);
        P.c3 = y, P.c4 = (e - 1.0) / y;
      } else {
        P.c3 = e;
      }
    }
  } else if (table) {
    if (a->cs2_stride < 1) OX_FAIL("ox_cell_viscosity: cs2_stride=%lld", (long long)a->cs2_stride);
    if (a->n_coef <= 0 || a->n_coef > (int64_t)0x7fffffff) OX_FAIL("ox_cell_viscosity: n_coef=%lld", (long long)a->n_coef);
    if (!a->cell_bin && a->n_coef != cells->n_cells)
      OX_FAIL("ox_cell_viscosity: n_coef=%lld coefficients for %lld cells and no cell_bin", (long long)a->n_coef,
              (long long)cells->n_cells);
  } else if (!(a->coefficient >= 0.0)) {
    OX_FAIL("ox_cell_viscosity: coefficient=%g", a->coefficient);
  }
  if (const ox_vandriest *vd = a->damping) {
    if (!vd->dist || !vd->nearest) OX_FAIL("ox_cell_viscosity: null argument (damping->dist, damping->nearest)");
    if (!(vd->nu > 0.0) || !std::isfinite(vd->nu)) OX_FAIL("ox_cell_viscosity: damping->nu=%g", vd->nu);
    if (!(vd->a_plus > 0.0) || !std::isfinite(vd->a_plus)) OX_FAIL("ox_cell_viscosity: damping->a_plus=%g", vd->a_plus);
    if (!vd->wss && (!(vd->u_tau >= 0.0) || !std::isfinite(vd->u_tau)))
      OX_FAIL("ox_cell_viscosity: damping->u_tau=%g", vd->u_tau);
    if (vd->n_facets < 1 || vd->n_facets > (int64_t)0x7fffffff)
      OX_FAIL("ox_cell_viscosity: damping->n_facets=%lld", (long long)vd->n_facets);
  }
  return 0;
}

}  // namespace

extern "C" int ox_cell_viscosity(const ox_cells *cells, const ox_viscosity_args *args, void *stream) {
  LawParams P{};
  if (nut_check(cells, args, P)) return -1;
  const int64_t nblk = ox_cell_blocks("ox_cell_viscosity", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const double c2 = args->coefficient * args->coefficient;
#define OX_NUT_CASE(GD, DG) \
  if (g == GD && args->degree == DG) return nut_model<GD, DG>(cells, args, c2, P, nblk, st);
  OX_FOR_GDIM_DEG(OX_NUT_CASE)
#undef OX_NUT_CASE
  OX_FAIL("ox_cell_viscosity: unsupported gdim=%d (degree=%d)", g, args->degree);
}
