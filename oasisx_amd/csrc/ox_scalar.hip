// Passive scalar transport: the Crank-Nicolson operator and right-hand side of a scalar group from the matrices the
// velocity step has at hand.
//
//   A   = M/dt + C(u_ab)/2 + nu K/2        what ox_assemble_first leaves in the velocity matrix BEFORE its Dirichlet rows
//   A_c = A + s K,  s = (kappa - nu)/2     the scalar's operator: same convection, its own diffusivity
//   b_c = (2/dt) M c_1 - A_c c_1 + b0_c    = (M/dt - C/2 - kappa K/2) c_1 + b0_c
//
// M, K, A and A_c share one SELL-64 pattern, so no element loop runs a second time: one streaming pass over the
// values.  One wave per slice (lane = row), 4 slices per 256-thread block, as k_spmv; per entry pair a lane loads 16 B
// of A, the pair of K and M (two 1-byte codes each through LDS copies of the dictionaries where both are frozen, 16 B
// each otherwise) and 8 B of columns, gathers c_1[col] once (NC columns) and stores 16 B of A_c.  A c_1 and M c_1 are
// summed in the stored entry order with one fused multiply-add per entry, from 0 -- the operations of k_spmv -- so the
// optional a_c1 = A_c c_1 equals ox_spmv(A_c, c_1) bit for bit and may be handed to the solver as its first mat-vec.
// No atomics, fixed order: two runs give the same bits.  Padding slots hold 0 in A and K and stay 0.
//
// Scalars that drive the flow and the flux through walls:
//   k_buoyancy_rows   b_first[r][i] += sum_t coef_t[i] (M d_t)[r],  d_t = (c1 + 0.5 (c1 - c2)) - ref of up to OX_MAXC
//                     coupled scalars, in one pass over M in the launch shape of k_scalar_rows
//   k_scalar_flux     q = -kappa n . gbar(c) on tagged exterior facets, one lane per facet as k_wall_stress
//
// Flux and Robin conditions of a scalar group, after k_scalar_rows and before the Dirichlet rows:
//   k_scalar_boundary one lane per touched row, shaped on k_outlet_backflow: the row's (condition facet, position among
//                     the facet's dofs) pairs in ascending order, the slots of A_c's value array from set-up.  With the
//                     facet rule (w_k, x_k), the nodal data interpolated on the facet and hq = h + beta max(-u_ab . n, 0):
//                       e_rs = (1/2) |f| sum_k w_k hq phi_r phi_s,   A_c[r][s] += e_rs,
//                       b_c[r][col] += |f| sum_k w_k (q_col + hq c_inf,col) phi_r - sum_s e_rs c_1[s][col]
//                     The lane owns its row of A_c and of b_c: no atomics, no LDS, a fixed order of sums.
#include "fe_tables_d.h"
#include "ox_element.h"

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));

template <int NC, bool DICT>
__global__ __launch_bounds__(256) void k_scalar_rows(ox_sell A, const double *__restrict__ Mv, const double *__restrict__ Kv,
                                                     const uint8_t *__restrict__ Mc, const uint8_t *__restrict__ Kc,
                                                     const double *__restrict__ Md, const double *__restrict__ Kd, int nMd,
                                                     int nKd, double *__restrict__ Acv, double s, double two_idt,
                                                     const double *__restrict__ c1, const double *__restrict__ b0,
                                                     double *__restrict__ b, double *__restrict__ a_c1) {
  __shared__ double dM[DICT ? 256 : 1], dK[DICT ? 256 : 1];
  if constexpr (DICT) {
    if ((int)threadIdx.x < nMd) dM[threadIdx.x] = Md[threadIdx.x];
    if ((int)threadIdx.x < nKd) dK[threadIdx.x] = Kd[threadIdx.x];
    __syncthreads();
  }
  // the blocks of one XCD (equal blockIdx % 8) take a contiguous eighth of the slices: neighbouring rows -- and their
  // c_1 gathers -- share an L2
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = ox_xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  if (li >= A.n_slices) return;
  const int slice = __builtin_amdgcn_readfirstlane(li);  // wave-uniform: scalar loads of the slice offsets
  const int64_t row = (int64_t)slice * 64 + lane;
  const int64_t base = A.slice_ptr[slice];
  const int npair = (int)((A.slice_ptr[slice + 1] - base) >> 7);
  const v2d *__restrict__ av = reinterpret_cast<const v2d *>(A.vals + base) + lane;
  const v2d *__restrict__ mv = reinterpret_cast<const v2d *>(Mv + base) + lane;
  const v2d *__restrict__ kv = reinterpret_cast<const v2d *>(Kv + base) + lane;
  const v2i *__restrict__ cp = reinterpret_cast<const v2i *>(A.cols + base) + lane;
  v2d *__restrict__ ov = reinterpret_cast<v2d *>(Acv + base) + lane;
  const unsigned short *__restrict__ mc = DICT ? reinterpret_cast<const unsigned short *>(Mc + base) + lane : nullptr;
  const unsigned short *__restrict__ kc = DICT ? reinterpret_cast<const unsigned short *>(Kc + base) + lane : nullptr;
  double sa[NC], sm[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) sa[c] = sm[c] = 0.0;
  // 4 entry pairs per turn, phase by phase (streams -> c_1 gathers -> arithmetic in the stored order -> stores): a turn
  // pays the two dependent memory rounds once (the epilogue of ox_assemble_first does the same)
  constexpr int EU = 4;
  for (int k0 = 0; k0 < npair; k0 += EU) {
    v2d a[EU], m[EU], kk[EU];
    v2i col[EU];
#pragma unroll
    for (int q = 0; q < EU; ++q) {
      const int k = min(k0 + q, npair - 1);  // unconditional loads inside the slice; the surplus is not used
      a[q] = __builtin_nontemporal_load(av + (size_t)k * 64);
      if constexpr (DICT) {
        const unsigned cm = __builtin_nontemporal_load(mc + (size_t)k * 64), ck = __builtin_nontemporal_load(kc + (size_t)k * 64);
        m[q].x = dM[cm & 0xff], m[q].y = dM[cm >> 8];
        kk[q].x = dK[ck & 0xff], kk[q].y = dK[ck >> 8];
      } else {
        m[q] = __builtin_nontemporal_load(mv + (size_t)k * 64);
        kk[q] = __builtin_nontemporal_load(kv + (size_t)k * 64);
      }
      col[q] = __builtin_nontemporal_load(cp + (size_t)k * 64);
    }
    double x0[EU][NC], x1[EU][NC];
#pragma unroll
    for (int q = 0; q < EU; ++q)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        x0[q][c] = c1[(size_t)col[q].x * NC + c];
        x1[q][c] = c1[(size_t)col[q].y * NC + c];
      }
#pragma unroll
    for (int q = 0; q < EU; ++q) {
      const int k = k0 + q;
      if (k < npair) {
        v2d v;
        v.x = fma(s, kk[q].x, a[q].x);
        v.y = fma(s, kk[q].y, a[q].y);
        __builtin_nontemporal_store(v, ov + (size_t)k * 64);
#pragma unroll
        for (int c = 0; c < NC; ++c) sa[c] = fma(v.x, x0[q][c], sa[c]);  // entry order and operations of k_spmv
#pragma unroll
        for (int c = 0; c < NC; ++c) sa[c] = fma(v.y, x1[q][c], sa[c]);
#pragma unroll
        for (int c = 0; c < NC; ++c) sm[c] = fma(m[q].y, x1[q][c], fma(m[q].x, x0[q][c], sm[c]));
      }
    }
  }
  if (row < A.n_rows) {
#pragma unroll
    for (int c = 0; c < NC; ++c) b[row * NC + c] = fma(two_idt, sm[c], -sa[c]) + b0[row * NC + c];
    if (a_c1) {
#pragma unroll
      for (int c = 0; c < NC; ++c) a_c1[row * NC + c] = sa[c];
    }
  }
}

template <int NC>
int launch(const ox_sell *A, const ox_sell *M, const ox_sell *K, double *acv, double s, double dt, const double *c1,
           const double *b0, double *b, double *a_c1, hipStream_t st) {
  const bool dict = M->vcode && K->vcode && M->vdict && K->vdict && M->n_dict > 0 && K->n_dict > 0 && M->n_dict <= 256 &&
                    K->n_dict <= 256;
  const unsigned nblk = (unsigned)((A->n_slices + 3) / 4);
  if (dict)
    hipLaunchKernelGGL((k_scalar_rows<NC, true>), dim3(nblk), dim3(256), 0, st, *A, M->vals, K->vals, M->vcode, K->vcode,
                       M->vdict, K->vdict, M->n_dict, K->n_dict, acv, s, 2.0 / dt, c1, b0, b, a_c1);
  else
    hipLaunchKernelGGL((k_scalar_rows<NC, false>), dim3(nblk), dim3(256), 0, st, *A, M->vals, K->vals, nullptr, nullptr,
                       nullptr, nullptr, 0, 0, acv, s, 2.0 / dt, c1, b0, b, a_c1);
  OX_LAUNCH_CHECK();
  return 0;
}

// ---- Boussinesq force ---------------------------------------------------------------------------------------------------
// The terms of one launch, by value in the kernel arguments: after unrolling every index into the table is a
// compile-time constant, so it stays in scalar registers (no scratch).
template <int NT>
struct BuoyTerms {
  ox_buoy_term t[NT];
};

// d_t[j]: the midpoint value c1 + 0.5 (c1 - c2) (c1 itself without a second level) minus the reference.  c1 == c2 gives
// c1 exactly, c == ref gives 0 exactly.
__device__ __forceinline__ double buoy_d(const ox_buoy_term &t, int j) {
  const size_t k = (size_t)j * t.nc + t.col;
  const double a = t.c1[k];
  const double e = t.c2 ? a + 0.5 * (a - t.c2[k]) : a;
  return e - t.ref;
}

// Launch shape of k_scalar_rows: one wave per slice (lane = row), 4 slices per block, the blocks of an XCD on contiguous
// slices.  Streamed per entry pair: 2 B of value codes (16 B of f64 values without a dictionary) and 8 B of columns;
// gathered: c1 and c2 of every term at the entry's column -- the terms of one scalar group read one (nc x 8 B) row of the
// group's blocks.  y_t = (M d_t)[row] is summed in the stored entry order with one fused multiply-add per entry, from 0:
// the operations of k_spmv on the vector d_t.  live: bit i set where component i has a nonzero coefficient; the others
// are neither read nor written.
template <int NT, bool DICT>
__global__ __launch_bounds__(256) void k_buoyancy_rows(ox_sell M, BuoyTerms<NT> T, int gdim, int live,
                                                       double *__restrict__ b) {
  __shared__ double dM[DICT ? 256 : 1];
  if constexpr (DICT) {
    if ((int)threadIdx.x < M.n_dict) dM[threadIdx.x] = M.vdict[threadIdx.x];
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = ox_xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  if (li >= M.n_slices) return;
  const int slice = __builtin_amdgcn_readfirstlane(li);
  const int64_t row = (int64_t)slice * 64 + lane;
  const int64_t base = M.slice_ptr[slice];
  const int npair = (int)((M.slice_ptr[slice + 1] - base) >> 7);
  const v2d *__restrict__ mv = reinterpret_cast<const v2d *>(M.vals + base) + lane;
  const v2i *__restrict__ cp = reinterpret_cast<const v2i *>(M.cols + base) + lane;
  const unsigned short *__restrict__ mc = DICT ? reinterpret_cast<const unsigned short *>(M.vcode + base) + lane : nullptr;
  double y[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) y[t] = 0.0;
  constexpr int EU = 4;  // entry pairs per turn: streams -> gathers -> arithmetic in the stored order, as k_scalar_rows
  for (int k0 = 0; k0 < npair; k0 += EU) {
    v2d m[EU];
    v2i col[EU];
#pragma unroll
    for (int q = 0; q < EU; ++q) {
      const int k = min(k0 + q, npair - 1);  // unconditional loads inside the slice; the surplus is not used
      if constexpr (DICT) {
        const unsigned cm = __builtin_nontemporal_load(mc + (size_t)k * 64);
        m[q].x = dM[cm & 0xff], m[q].y = dM[cm >> 8];
      } else {
        m[q] = __builtin_nontemporal_load(mv + (size_t)k * 64);
      }
      col[q] = __builtin_nontemporal_load(cp + (size_t)k * 64);
    }
    double d0[EU][NT], d1[EU][NT];
#pragma unroll
    for (int q = 0; q < EU; ++q)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        d0[q][t] = buoy_d(T.t[t], col[q].x);
        d1[q][t] = buoy_d(T.t[t], col[q].y);
      }
#pragma unroll
    for (int q = 0; q < EU; ++q)
      if (k0 + q < npair) {
#pragma unroll
        for (int t = 0; t < NT; ++t) y[t] = fma(m[q].y, d1[q][t], fma(m[q].x, d0[q][t], y[t]));
      }
  }
  if (row < M.n_rows) {
#pragma unroll
    for (int i = 0; i < OX_MAXC; ++i)
      if (i < gdim && ((live >> i) & 1)) {
        double s = T.t[0].coef[i] * y[0];
#pragma unroll
        for (int t = 1; t < NT; ++t) s = fma(T.t[t].coef[i], y[t], s);  // terms ascending
        b[row * gdim + i] += s;
      }
  }
}

template <int NT>
int launch_buoyancy(const ox_sell *M, int gdim, const ox_buoy_term *terms, double *b, hipStream_t st) {
  BuoyTerms<NT> T;
  int live = 0;
  for (int t = 0; t < NT; ++t) {
    T.t[t] = terms[t];
    for (int i = 0; i < gdim; ++i)
      if (terms[t].coef[i] != 0.0) live |= 1 << i;
  }
  if (!live) return 0;  // nothing to add to any component
  const bool dict = M->vcode && M->vdict && M->n_dict > 0 && M->n_dict <= 256;
  const unsigned nblk = (unsigned)((M->n_slices + 3) / 4);
  if (ox_prof_on) ox_prof_start(OX_TAG_BUOYANCY_ROWS, st, 2 * NT + (dict ? 1 : 0));
  if (dict) hipLaunchKernelGGL((k_buoyancy_rows<NT, true>), dim3(nblk), dim3(256), 0, st, *M, T, gdim, live, b);
  else hipLaunchKernelGGL((k_buoyancy_rows<NT, false>), dim3(nblk), dim3(256), 0, st, *M, T, gdim, live, b);
  if (ox_prof_on) ox_prof_stop(st);
  OX_LAUNCH_CHECK();
  return 0;
}

// ---- diffusive flux through exterior facets -----------------------------------------------------------------------------
// One lane per facet, records as for k_wall_stress.  Streamed: the record (8 B) and the three results (and, with
// weight > 0, the read-modify-write of the accumulator); gathered: the cell's dof list, geometry record and ND values of
// column col of c.  The facet means of the basis and of its gradient are compile-time constants: identically-zero
// entries cost nothing; the local facet selects one of GDIM + 1 instantiations of the contraction.
// CELLS (a solver with a viscosity model): the coefficient is kappa + nut[cell] inv_sct, one more
// gathered double per facet; the other instantiation reads neither argument and keeps the code it had.
template <int GDIM, int DEG, bool CELLS = false>
__global__ __launch_bounds__(256) void k_scalar_flux(ox_cells cells, const int32_t *__restrict__ dofs, int64_t n_facets,
                                                     const int2 *__restrict__ rec, const double *__restrict__ c, int nc,
                                                     int col, double kappa, double weight, double *__restrict__ q,
                                                     double *__restrict__ fq, double *__restrict__ cbar,
                                                     double *__restrict__ acc_q, const double *__restrict__ nut = nullptr,
                                                     double inv_sct = 0.0) {
  constexpr int ND = ox_nd(GDIM, DEG);
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= n_facets) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  double qv = qnan, fv = qnan, cb = qnan;
  const int2 r = rec[f];
  // a record outside the tables reads nothing and leaves NaN
  if (r.x >= 0 && (int64_t)r.x < cells.n_cells && r.y >= 0 && r.y <= GDIM) {
    const int64_t e = r.x;
    int32_t dd[ND];
    ox_load_dofs<ND>(dofs, e, dd);
    double G[GDIM + 1][GDIM], adet;
    ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
    double cc[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) cc[i] = c[(size_t)dd[i] * nc + col];
    // tb[b] = sum_i c_i mean_f(dphi_i/dlambda_b) and the mean of c on the local facet, in dof order; Ga = grad lambda_a
    double tb[GDIM + 1] = {}, mean = 0.0, Ga[GDIM] = {};
    ox_facet_dispatch<GDIM>(r.y, [&](auto facet) {
      constexpr int A = decltype(facet)::value;
#pragma unroll
      for (int i = 0; i < ND; ++i) {
#pragma unroll
        for (int bb = 0; bb <= GDIM; ++bb)
          if (ox_dphif<GDIM, DEG>()[A][i][bb] != 0.0) tb[bb] = fma(cc[i], ox_dphif<GDIM, DEG>()[A][i][bb], tb[bb]);
        if (ox_phif<GDIM, DEG>()[A][i] != 0.0) mean = fma(cc[i], ox_phif<GDIM, DEG>()[A][i], mean);
      }
#pragma unroll
      for (int d = 0; d < GDIM; ++d) Ga[d] = G[A][d];
    });
    double n[GDIM], area;
    ox_facet_normal<GDIM>(Ga, adet, n, area);
    double gn = 0.0;  // n . gbar, gbar[k] = sum_b tb[b] G[b][k]
#pragma unroll
    for (int k = 0; k < GDIM; ++k) {
      double g = 0.0;
#pragma unroll
      for (int bb = 0; bb <= GDIM; ++bb) g = fma(tb[bb], G[bb][k], g);
      gn = fma(n[k], g, gn);
    }
    if constexpr (CELLS) qv = -fma(nut[e], inv_sct, kappa) * gn;
    else qv = -kappa * gn;
    fv = area * qv;
    cb = mean;
  }
  q[f] = qv;
  fq[f] = fv;
  cbar[f] = cb;
  if (weight > 0.0) acc_q[f] = __dadd_rn(acc_q[f], __dmul_rn(weight, qv));
}

// ---- flux and Robin conditions ------------------------------------------------------------------------------------------
// One lane per touched row.  Streamed per pair: 8 B of (facet, position) and, with ROBIN, NFD slots; gathered: the
// facet's record and geometry, its nodal data (q, and with ROBIN h and c_inf: rows of NFD x nc doubles, read once per
// pair) and, with ROBIN, the facet's dofs and c_1 there; with ADV u_ab at those dofs.  Live over the rule loop: hn, un,
// ent, dvf (NFD each, ROBIN / ADV only), one column's qn and cn (NFD doubles each) and acc (OX_MAXC doubles): nothing
// spills in any instance (profiles/scalar_bc_kernel_resources.txt).  A first form re-read the nodal data per rule point
// to save registers and paid a round of loads per point: 0.155 against 0.076 ms for the backflow kernel on one face.
// ROBIN = false reads neither A_c, c_1 nor u_ab; only ADV = true reads u_ab.
template <int GDIM, int DU, bool ROBIN, bool ADV>
__global__ __launch_bounds__(256) void k_scalar_boundary(ox_cells cells, const int32_t *__restrict__ dofs,
                                                         ox_scalar_bc_args P) {
  static_assert(ROBIN || !ADV, "the advective part belongs to a Robin condition");
  using O = ox_facet_rule<GDIM, DU>;
  constexpr int ND = ox_nd(GDIM, DU), NFD = O::NFD;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n_rows) return;
  const int nc = P.nc;
  double acc[OX_MAXC];
#pragma unroll
  for (int c = 0; c < OX_MAXC; ++c) acc[c] = 0.0;
  for (int64_t k = P.row_ptr[i]; k < P.row_ptr[i + 1]; ++k) {
    const int64_t fi = P.pair_facet[k];
    const int jr = P.pair_loc[k];
    if (fi < 0 || fi >= P.n_facets || jr < 0 || jr >= NFD) continue;  // a pair outside the tables adds nothing
    const int2 r = reinterpret_cast<const int2 *>(P.facet_rec)[fi];
    if (!(r.x >= 0 && (int64_t)r.x < cells.n_cells && r.y >= 0 && r.y <= GDIM)) continue;
    const int64_t e = r.x;
    const int a = r.y;
    double n[GDIM], area;
    ox_facet_geometry<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), a, n, area);
    const double *__restrict__ qf = P.q + (size_t)fi * NFD * nc;
    const double *__restrict__ hf = ROBIN ? P.h + (size_t)fi * NFD : nullptr;
    const double *__restrict__ cf = ROBIN ? P.c_inf + (size_t)fi * NFD * nc : nullptr;
    size_t dvf[NFD];
    double un[NFD], ent[NFD], hn[NFD];
    double beta = 0.0;
    if constexpr (ROBIN) {
#pragma unroll
      for (int j = 0; j < NFD; ++j) {
        dvf[j] = (size_t)dofs[(size_t)e * ND + O::fd(a, j)];
        hn[j] = hf[j];
        ent[j] = 0.0;
      }
    }
    if constexpr (ADV) {
      beta = P.beta[fi];
#pragma unroll
      for (int j = 0; j < NFD; ++j) {
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < GDIM; ++d) s = fma(P.uab[dvf[j] * GDIM + d], n[d], s);
        un[j] = s;
      }
    }
    // column by column: the column's nodal q and c_inf are loaded once and stay in registers over the rule loop (no load
    // inside it); hq is formed again per column -- 2 NFD multiply-adds per point, against a round of gathers -- by the same
    // operations, so every column sees the same bits; the entries e_rs are summed in the first column's loop
#pragma unroll
    for (int c = 0; c < OX_MAXC; ++c)
      if (c < nc) {
        double qn[NFD], cn[NFD];
#pragma unroll
        for (int j = 0; j < NFD; ++j) {
          qn[j] = qf[j * nc + c];
          if constexpr (ROBIN) cn[j] = cf[j * nc + c];
        }
        double load = 0.0;
        for (int q = 0; q < O::NQ; ++q) {
          const double gr = O::w(q) * O::phi(q, jr);
          double hq = 0.0;
          if constexpr (ROBIN) {
#pragma unroll
            for (int j = 0; j < NFD; ++j) hq = fma(hn[j], O::phi(q, j), hq);
          }
          if constexpr (ADV) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NFD; ++j) s = fma(O::phi(q, j), un[j], s);
            hq = fma(beta, fmax(-s, 0.0), hq);
          }
          double v = 0.0;
#pragma unroll
          for (int j = 0; j < NFD; ++j) v = fma(qn[j], O::phi(q, j), v);
          if constexpr (ROBIN) {
            double ci = 0.0;
#pragma unroll
            for (int j = 0; j < NFD; ++j) ci = fma(cn[j], O::phi(q, j), ci);
            v = fma(hq, ci, v);
          }
          load = fma(gr, v, load);
          if (ROBIN && c == 0) {
            const double g2 = gr * hq;
#pragma unroll
            for (int j = 0; j < NFD; ++j) ent[j] = fma(g2, O::phi(q, j), ent[j]);
          }
        }
        acc[c] = fma(area, load, acc[c]);
      }
    if constexpr (ROBIN) {
      const double hc = 0.5 * area;
#pragma unroll
      for (int j = 0; j < NFD; ++j) {
        const double v = hc * ent[j];
        const int64_t off = P.pair_off[(size_t)k * NFD + j];
        if (off >= 0 && off < P.a_size) P.a_vals[off] += v;
#pragma unroll
        for (int c = 0; c < OX_MAXC; ++c)
          if (c < nc) acc[c] = fma(-v, P.c1[dvf[j] * nc + c], acc[c]);
      }
    }
  }
  const int64_t row = P.rows[i];
  if (row < 0 || row >= P.n_dofs) return;
#pragma unroll
  for (int c = 0; c < OX_MAXC; ++c)
    if (c < nc) P.b[(size_t)row * nc + c] += acc[c];
}

}  // namespace

extern "C" int ox_scalar_rows(const ox_sell *A, const ox_sell *M, const ox_sell *K, const ox_sell *Ac, double s, double dt,
                              int ncomp, const double *c1, const double *b0, double *b, double *a_c1, void *stream) {
  if (!A || !M || !K || !Ac || !A->vals || !M->vals || !K->vals || !Ac->vals || !c1 || !b0 || !b)
    OX_FAIL("ox_scalar_rows: null argument");
  if (M->slice_ptr != A->slice_ptr || K->slice_ptr != A->slice_ptr || Ac->slice_ptr != A->slice_ptr)
    OX_FAIL("ox_scalar_rows: A, M, K and A_c must share one sparsity pattern");
  if (Ac->vals == A->vals || Ac->vals == M->vals || Ac->vals == K->vals)
    OX_FAIL("ox_scalar_rows: A_c needs a value array of its own");
  if (!(dt > 0.0)) OX_FAIL("ox_scalar_rows: dt=%g", dt);
  if (ncomp < 1 || ncomp > OX_MAXC) OX_FAIL("ox_scalar_rows: ncomp=%d", ncomp);
  if (A->n_slices <= 0) return 0;
  hipStream_t st = ox_stream(stream);
  switch (ncomp) {
    case 1: return launch<1>(A, M, K, Ac->vals, s, dt, c1, b0, b, a_c1, st);
    case 2: return launch<2>(A, M, K, Ac->vals, s, dt, c1, b0, b, a_c1, st);
    default: return launch<3>(A, M, K, Ac->vals, s, dt, c1, b0, b, a_c1, st);
  }
}

extern "C" int ox_buoyancy_rows(const ox_sell *M, int gdim, int n_terms, const ox_buoy_term *terms, double *b,
                                void *stream) {
  if (!M || !M->vals || !M->cols || !M->slice_ptr || !terms || !b) OX_FAIL("ox_buoyancy_rows: null argument");
  if (gdim != 2 && gdim != 3) OX_FAIL("ox_buoyancy_rows: gdim=%d", gdim);
  if (n_terms < 1 || n_terms > OX_MAXC) OX_FAIL("ox_buoyancy_rows: n_terms=%d", n_terms);
  for (int t = 0; t < n_terms; ++t) {
    if (!terms[t].c1) OX_FAIL("ox_buoyancy_rows: term %d has no c1", t);
    if (terms[t].nc < 1 || terms[t].col < 0 || terms[t].col >= terms[t].nc)
      OX_FAIL("ox_buoyancy_rows: term %d: column %d of %d", t, (int)terms[t].col, (int)terms[t].nc);
  }
  if (M->n_slices <= 0) return 0;
  hipStream_t st = ox_stream(stream);
  switch (n_terms) {
    case 1: return launch_buoyancy<1>(M, gdim, terms, b, st);
    case 2: return launch_buoyancy<2>(M, gdim, terms, b, st);
    default: return launch_buoyancy<3>(M, gdim, terms, b, st);
  }
}

extern "C" int ox_scalar_flux(int degree, const ox_cells *cells, const int32_t *cell_dofs, int64_t n_facets,
                              const int32_t *facet_rec, const double *c, int nc, int col, double kappa, double weight,
                              double *q, double *fq, double *cbar, double *acc_q, void *stream) {
  if (!cells || !cells->geom || !cell_dofs || !facet_rec || !c || !q || !fq || !cbar) OX_FAIL("ox_scalar_flux: null argument");
  if (nc < 1 || col < 0 || col >= nc) OX_FAIL("ox_scalar_flux: column %d of %d", col, nc);
  if (weight > 0.0 && !acc_q) OX_FAIL("ox_scalar_flux: weight > 0 without an accumulator");
  if (!(weight >= 0.0)) OX_FAIL("ox_scalar_flux: weight=%g", weight);
  if (n_facets <= 0) return 0;
  if (n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_scalar_flux: %lld facets, %lld cells", (long long)n_facets, (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_facets + 255) / 256);
#define OX_SCALAR_FLUX_CASE(GD, DG)                                                                                   \
  if (g == GD && degree == DG) {                                                                                      \
    if (ox_prof_on) ox_prof_start(OX_TAG_SCALAR_FLUX, st, n_facets);                                                  \
    hipLaunchKernelGGL((k_scalar_flux<GD, DG>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, n_facets,            \
                       reinterpret_cast<const int2 *>(facet_rec), c, nc, col, kappa, weight, q, fq, cbar, acc_q);     \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_SCALAR_FLUX_CASE)
#undef OX_SCALAR_FLUX_CASE
  OX_FAIL("ox_scalar_flux: unsupported gdim=%d, P%d", g, degree);
}

extern "C" int ox_scalar_flux_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, int64_t n_facets,
                                    const int32_t *facet_rec, const double *c, int nc, int col, double kappa,
                                    const double *nut, double inv_sct, double weight, double *q, double *fq, double *cbar,
                                    double *acc_q, void *stream) {
  if (!cells || !cells->geom || !cell_dofs || !facet_rec || !c || !q || !fq || !cbar || !nut)
    OX_FAIL("ox_scalar_flux_cells: null argument");
  if (nc < 1 || col < 0 || col >= nc) OX_FAIL("ox_scalar_flux_cells: column %d of %d", col, nc);
  if (weight > 0.0 && !acc_q) OX_FAIL("ox_scalar_flux_cells: weight > 0 without an accumulator");
  if (!(inv_sct >= 0.0) || inv_sct > 1.0e300) OX_FAIL("ox_scalar_flux_cells: inv_sct=%g", inv_sct);
  if (!(weight >= 0.0)) OX_FAIL("ox_scalar_flux_cells: weight=%g", weight);
  if (n_facets <= 0) return 0;
  if (n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_scalar_flux_cells: %lld facets, %lld cells", (long long)n_facets, (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((n_facets + 255) / 256);
#define OX_SCALAR_FLUXC_CASE(GD, DG)                                                                                  \
  if (g == GD && degree == DG) {                                                                                      \
    if (ox_prof_on) ox_prof_start(OX_TAG_SCALAR_FLUX, st, n_facets);                                                  \
    hipLaunchKernelGGL((k_scalar_flux<GD, DG, true>), dim3(nblk), dim3(256), 0, st, *cells, cell_dofs, n_facets,      \
                       reinterpret_cast<const int2 *>(facet_rec), c, nc, col, kappa, weight, q, fq, cbar, acc_q, nut, \
                       inv_sct);                                                                                      \
    if (ox_prof_on) ox_prof_stop(st);                                                                                 \
    OX_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                         \
  }
  OX_FOR_GDIM_DEG(OX_SCALAR_FLUXC_CASE)
#undef OX_SCALAR_FLUXC_CASE
  OX_FAIL("ox_scalar_flux_cells: unsupported gdim=%d, P%d", g, degree);
}

extern "C" int ox_scalar_boundary(const ox_cells *cells, const int32_t *cell_dofs, const ox_scalar_bc_args *args,
                                  void *stream) {
  if (!cells || !cells->geom || !cell_dofs || !args) OX_FAIL("ox_scalar_boundary: null argument");
  const ox_scalar_bc_args &P = *args;
  if (!P.rows || !P.row_ptr || !P.pair_facet || !P.pair_loc || !P.facet_rec || !P.q || !P.b)
    OX_FAIL("ox_scalar_boundary: null argument");
  if (P.adv && !P.robin) OX_FAIL("ox_scalar_boundary: adv without robin");
  if (P.robin && (!P.pair_off || !P.h || !P.c_inf || !P.c1 || !P.a_vals || P.a_size <= 0))
    OX_FAIL("ox_scalar_boundary: a Robin pass without its arrays");
  if (P.adv && (!P.beta || !P.uab)) OX_FAIL("ox_scalar_boundary: an advective pass without beta or u_ab");
  if (P.nc < 1 || P.nc > OX_MAXC) OX_FAIL("ox_scalar_boundary: nc=%d", P.nc);
  if (P.n_rows <= 0) return 0;
  if (P.n_rows > (int64_t)0x7fffffff || P.n_facets > (int64_t)0x7fffffff || cells->n_cells > (int64_t)0x7fffffff)
    OX_FAIL("ox_scalar_boundary: %lld rows, %lld facets, %lld cells", (long long)P.n_rows, (long long)P.n_facets,
            (long long)cells->n_cells);
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const unsigned nblk = (unsigned)((P.n_rows + 255) / 256);
#define OX_SCALAR_BC_CASE(GD, DG)                                                                                      \
  if (g == GD && P.degree == DG) {                                                                                     \
    if (ox_prof_on) ox_prof_start(OX_TAG_SCALAR_BOUNDARY, st, P.n_rows);                                               \
    if (P.adv) hipLaunchKernelGGL((k_scalar_boundary<GD, DG, true, true>), dim3(nblk), dim3(256), 0, st, *cells,       \
                                  cell_dofs, P);                                                                       \
    else if (P.robin) hipLaunchKernelGGL((k_scalar_boundary<GD, DG, true, false>), dim3(nblk), dim3(256), 0, st,       \
                                         *cells, cell_dofs, P);                                                        \
    else hipLaunchKernelGGL((k_scalar_boundary<GD, DG, false, false>), dim3(nblk), dim3(256), 0, st, *cells,           \
                            cell_dofs, P);                                                                             \
    if (ox_prof_on) ox_prof_stop(st);                                                                                  \
    OX_LAUNCH_CHECK();                                                                                                 \
    return 0;                                                                                                          \
  }
  OX_FOR_GDIM_DEG(OX_SCALAR_BC_CASE)
#undef OX_SCALAR_BC_CASE
  OX_FAIL("ox_scalar_boundary: unsupported gdim=%d, P%d", g, P.degree);
}

// ---- SUPG stabilisation ----------------------------------------------------------------------------
// Per cell c, one lane, no LDS, no atomics: the frozen velocity w_c = u_ab at the centroid (the centroid values of the basis,
// fe_tables_d.h, in the dof order of k_drag_sigma) and Shakib's parameter
//   tau_c = scale ([time_term] (2/dt)^2 + (k q_c)^2 + (2 k^2 kappa_c g_c)^2)^(-1/2),
//   q_c = sum_a |w_c . G[a]|,  g_c = sum_a |G[a]|^2,  kappa_c = kappa + inv_sct nut_c,  k = the element's degree.
// Nothing is divided by |w|: w = 0 gives a finite tau (0 where every term under the root is 0); a velocity that is not finite
// is shown, not clipped: NaN.  rec is a structure of arrays in kernel cell order: rec[d][c] = w_c[d], rec[GDIM][c] = tau_c.
namespace {

template <int GDIM, int DEG>
__global__ __launch_bounds__(256) void k_supg_cells(ox_cells cells, const int32_t *__restrict__ cell_dofs,
                                                    const double *__restrict__ uab, const double *__restrict__ nut,
                                                    double kappa, double inv_sct, double t2, double scale,
                                                    double *__restrict__ rec) {
  constexpr int ND = ox_nd(GDIM, DEG);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cells.n_cells) return;
  int32_t dd[ND];
  ox_load_dofs<ND>(cell_dofs, e, dd);
  double G[GDIM + 1][GDIM], adet;
  ox_load_geom<GDIM>(cells.geom + (size_t)e * ox_gs(GDIM), G, adet);
  double uc[ND][GDIM];
  ox_gather<ND, GDIM>(dd, uab, uc);
  const auto phic = [](int i) -> double { OX_FE_PICK(GDIM, DEG, OX_PHIC, [i]); };
  double w[GDIM] = {};
#pragma unroll
  for (int i = 0; i < ND; ++i)
    if (phic(i) != 0.0) {
#pragma unroll
      for (int d = 0; d < GDIM; ++d) w[d] = fma(uc[i][d], phic(i), w[d]);
    }
  double q = 0.0, g = 0.0;
#pragma unroll
  for (int a = 0; a <= GDIM; ++a) {
    double wa = 0.0;
#pragma unroll
    for (int d = 0; d < GDIM; ++d) {
      wa = fma(w[d], G[a][d], wa);
      g = fma(G[a][d], G[a][d], g);
    }
    q += fabs(wa);
  }
  const double kap = nut ? fma(inv_sct, nut[e], kappa) : kappa;
  const double cq = DEG * q, cd = (2.0 * DEG * DEG) * kap * g;
  const double r = fma(cd, cd, fma(cq, cq, t2));
  double tau = r > 0.0 ? scale / sqrt(r) : 0.0;
  if (!isfinite(r)) tau = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int d = 0; d < GDIM; ++d) rec[(size_t)d * cells.n_cells + e] = w[d];
  rec[(size_t)GDIM * cells.n_cells + e] = tau;
}

}  // namespace

extern "C" int ox_supg_cells(int degree, const ox_cells *cells, const int32_t *cell_dofs, const double *uab,
                             const double *nut, double kappa, double inv_sct, double dt, double scale, int time_term,
                             double *rec, void *stream) {
  if (!cells || !cells->geom || !cell_dofs || !uab || !rec) OX_FAIL("ox_supg_cells: null argument");
  if (!(dt > 0.0)) OX_FAIL("ox_supg_cells: dt=%g", dt);
  if (!(scale > 0.0) || !(kappa >= 0.0) || !(inv_sct >= 0.0))
    OX_FAIL("ox_supg_cells: scale=%g, kappa=%g, 1/Sc_t=%g", scale, kappa, inv_sct);
  const int64_t nblk = ox_cell_blocks("ox_supg_cells", cells);
  if (nblk <= 0) return (int)nblk;
  hipStream_t st = ox_stream(stream);
  const int g = cells->gdim;
  const double t2 = time_term ? (2.0 / dt) * (2.0 / dt) : 0.0;
#define OX_SUPG_CELLS_CASE(GD, DG)                                                                                   \
  if (g == GD && degree == DG) {                                                                                     \
    if (ox_prof_on) ox_prof_start(OX_TAG_SUPG_CELLS, st, cells->n_cells);                                            \
    hipLaunchKernelGGL((k_supg_cells<GD, DG>), dim3((unsigned)nblk), dim3(256), 0, st, *cells, cell_dofs, uab, nut,  \
                       kappa, inv_sct, t2, scale, rec);                                                              \
    if (ox_prof_on) ox_prof_stop(st);                                                                                \
    OX_LAUNCH_CHECK();                                                                                               \
    return 0;                                                                                                        \
  }
  OX_FOR_GDIM_DEG(OX_SUPG_CELLS_CASE)
#undef OX_SUPG_CELLS_CASE
  OX_FAIL("ox_supg_cells: unsupported gdim=%d, P%d", g, degree);
}
