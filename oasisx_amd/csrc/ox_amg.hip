// Smoothed-aggregation AMG V-cycle (PETSc's PCGAMG with its Chebyshev-Jacobi level smoothers) on SELL-64 levels.
//
// A cycle is a fixed program of PHASES, laid out once by ox_mg_create: every phase is a row-local operation with at
// most one sparse row product, lane = row over SELL-64 like the other kernels of the library:
//   MG_S0        first smoothing step from x = 0 (no mat-vec):     d = c_r D^-1 b;  x = d
//   MG_STEP      Chebyshev step, mat-vec fused:                    r = D^-1 (b - A x_in);  d = c_d d + c_r r;  x_out = x_in + d
//   MG_STEPY     the same with y = A x_in from ox_spmv (level 0: the caller's operator through all its storage levels)
//   MG_SPMV      y = A x                                            (the residual's product)
//   MG_RESTRICT  b_c = R (b - y), R multiplied by its own rows (no atomics), fused with MG_S0 of the coarse level
//   MG_PROLONG   x_out = x_in + P x_c
//   MG_COARSE    x_c = A_c^-1 b_c with the dense inverse
// Every sum runs in a fixed order (the row's entries in storage order): identical runs give identical bits.  The phases
// of the levels of at most `tail_rows` rows and the coarse solve run in ONE single-workgroup launch (k_mg_tail): a
// launch costs ~3.5 us, more than such a phase's work.  Every kernel returns at once when the Krylov state says `done`.
#include <vector>

#include "ox_kernels.h"

enum { MG_S0 = 0, MG_STEP, MG_STEPY, MG_SPMV, MG_RESTRICT, MG_PROLONG, MG_COARSE };

struct MgMat {
  const int64_t *sp;
  const int32_t *cols;
  const double *vals;
};

struct MgPhase {
  int kind;
  int level;
  int64_t n;  // rows of the phase (MG_COARSE: n_c, the dense inverse's order)
  MgMat M;    // A (steps, MG_SPMV), R (MG_RESTRICT), P (MG_PROLONG); MG_COARSE: vals = the inverse
  const double *dinv, *b, *y, *xin, *xc;
  double *xout, *d, *out;
  double cd, cr;
  // MG_RESTRICT: MG_S0 of the coarse level (d2 == nullptr: the coarse level is the coarsest)
  const double *dinv2;
  double *x2, *d2;
  double cr2;
};

// level 0's right-hand side and result change from call to call: phases name them by these tags
#define MG_B0 (reinterpret_cast<double *>(16))
#define MG_Z0 (reinterpret_cast<double *>(32))
__device__ __forceinline__ const double *mg_res(const double *p, const double *b0, double *z0) {
  return p == MG_B0 ? b0 : (p == MG_Z0 ? z0 : p);
}
__device__ __forceinline__ double *mg_resw(double *p, double *z0) { return p == MG_Z0 ? z0 : p; }

// (A x)_row, entries in storage order (padding: value 0 at a valid column)
__device__ __forceinline__ double mg_row(const MgMat &M, int64_t row, const double *__restrict__ x) {
  const int64_t s = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t e = M.sp[s + 1];
  double acc = 0.0;
  for (int64_t o = M.sp[s] + lane * OX_KV; o < e; o += 64 * OX_KV) {
    const double2 v = *reinterpret_cast<const double2 *>(M.vals + o);
    const int2 c = *reinterpret_cast<const int2 *>(M.cols + o);
    acc = fma(v.x, x[c.x], acc);
    acc = fma(v.y, x[c.y], acc);
  }
  return acc;
}
// (M (b - y))_row
__device__ __forceinline__ double mg_row_diff(const MgMat &M, int64_t row, const double *__restrict__ b,
                                              const double *__restrict__ y) {
  const int64_t s = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t e = M.sp[s + 1];
  double acc = 0.0;
  for (int64_t o = M.sp[s] + lane * OX_KV; o < e; o += 64 * OX_KV) {
    const double2 v = *reinterpret_cast<const double2 *>(M.vals + o);
    const int2 c = *reinterpret_cast<const int2 *>(M.cols + o);
    acc = fma(v.x, b[c.x] - y[c.x], acc);
    acc = fma(v.y, b[c.y] - y[c.y], acc);
  }
  return acc;
}

__device__ __forceinline__ void mg_phase_row(const MgPhase &P, int64_t row, const double *b0, double *z0) {
  switch (P.kind) {
    case MG_S0: {
      const double dd = P.cr * (P.dinv[row] * mg_res(P.b, b0, z0)[row]);
      P.d[row] = dd;
      mg_resw(P.xout, z0)[row] = dd;
      break;
    }
    case MG_STEP:
    case MG_STEPY: {
      const double *xin = P.xin;
      const double y = P.kind == MG_STEP ? mg_row(P.M, row, xin) : P.y[row];
      const double r = P.dinv[row] * (mg_res(P.b, b0, z0)[row] - y);
      const double dd = P.cd == 0.0 ? P.cr * r : fma(P.cd, P.d[row], P.cr * r);
      P.d[row] = dd;
      mg_resw(P.xout, z0)[row] = xin[row] + dd;
      break;
    }
    case MG_SPMV:
      P.out[row] = mg_row(P.M, row, P.xin);
      break;
    case MG_RESTRICT: {
      const double s = mg_row_diff(P.M, row, mg_res(P.b, b0, z0), P.y);
      P.out[row] = s;
      if (P.d2) {
        const double dd = P.cr2 * (P.dinv2[row] * s);
        P.d2[row] = dd;
        P.x2[row] = dd;
      }
      break;
    }
    case MG_PROLONG:
      mg_resw(P.xout, z0)[row] = P.xin[row] + mg_row(P.M, row, P.xc);
      break;
    case MG_COARSE: {
      const double *__restrict__ a = P.M.vals + row * P.n;
      const double *__restrict__ b = mg_res(P.b, b0, z0);
      double s = 0.0;
      for (int64_t j = 0; j < P.n; ++j) s = fma(a[j], b[j], s);
      mg_resw(P.out, z0)[row] = s;
      break;
    }
  }
}

__global__ __launch_bounds__(256) void k_mg_phase(MgPhase P, const double *b0, double *z0, const int *done) {
  if (done && *done) return;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < P.n) mg_phase_row(P, row, b0, z0);
}

#define OX_MG_TAIL_T 1024
// the small levels: every phase by the whole workgroup (a wave takes whole slices), a workgroup barrier between phases
__global__ __launch_bounds__(OX_MG_TAIL_T) void k_mg_tail(const MgPhase *__restrict__ ph, int nph, const double *b0,
                                                          double *z0, const int *done) {
  if (done && *done) return;
  for (int i = 0; i < nph; ++i) {
    const MgPhase P = ph[i];
    for (int64_t row = threadIdx.x; row < P.n; row += OX_MG_TAIL_T) mg_phase_row(P, row, b0, z0);
    __threadfence_block();
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// host side
enum { OP_PHASE = 0, OP_SPMV0, OP_TAIL };
struct MgOp {
  int kind;
  MgPhase ph;        // OP_PHASE
  double *x, *y;     // OP_SPMV0: y = A_0 x with the caller's operator
};

struct ox_mg {
  int n_levels;
  ox_mg_level lv[OX_MG_MAX_LEVELS];
  std::vector<MgOp> ops;
  MgPhase *tail_dev;  // device copy of the tail's phases
  int n_tail;
  void *mem;          // the level vectors
  int kernels;
};

#define OX_MG_TAIL_ROWS_DEFAULT 2048

static MgMat mg_mat(const ox_sell &S) { return MgMat{S.slice_ptr, S.cols, S.vals}; }

extern "C" int ox_mg_create(int n_levels, const ox_mg_level *levels, const double *coarse_inv, int tail_rows, ox_mg **out) {
  if (!levels || !coarse_inv || !out) OX_FAIL("ox_mg_create: null argument");
  if (n_levels < 1 || n_levels > OX_MG_MAX_LEVELS) OX_FAIL("ox_mg_create: %d levels (1..%d)", n_levels, OX_MG_MAX_LEVELS);
  *out = nullptr;
  const int c = n_levels - 1;
  for (int l = 0; l < n_levels; ++l) {
    const ox_mg_level &L = levels[l];
    if (L.n_rows < 1 || !L.dinv) OX_FAIL("ox_mg_create: level %d: %lld rows / no diagonal", l, (long long)L.n_rows);
    if (l == c) continue;
    const int64_t nc = levels[l + 1].n_rows;
    if (L.degree < 1 || L.degree > OX_MG_MAX_DEGREE) OX_FAIL("ox_mg_create: level %d: degree %d", l, L.degree);
    if (L.A.n_rows != L.n_rows || L.A.n_cols < L.n_rows || !L.A.slice_ptr || !L.A.cols || !L.A.vals)
      OX_FAIL("ox_mg_create: level %d: operator of %lld x %lld rows", l, (long long)L.A.n_rows, (long long)L.A.n_cols);
    if (L.P.n_rows != L.n_rows || L.P.n_cols != nc || !L.P.slice_ptr || !L.P.cols || !L.P.vals)
      OX_FAIL("ox_mg_create: level %d: prolongation %lld x %lld, expected %lld x %lld", l, (long long)L.P.n_rows,
              (long long)L.P.n_cols, (long long)L.n_rows, (long long)nc);
    if (L.R.n_rows != nc || L.R.n_cols != L.n_rows || !L.R.slice_ptr || !L.R.cols || !L.R.vals)
      OX_FAIL("ox_mg_create: level %d: restriction %lld x %lld, expected %lld x %lld", l, (long long)L.R.n_rows,
              (long long)L.R.n_cols, (long long)nc, (long long)L.n_rows);
  }
  if (levels[c].n_rows > 4096) OX_FAIL("ox_mg_create: coarsest level of %lld rows (dense inverse)", (long long)levels[c].n_rows);
  const int64_t T = tail_rows > 0 ? tail_rows : OX_MG_TAIL_ROWS_DEFAULT;

  ox_mg *mg = new ox_mg();
  mg->n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) mg->lv[l] = levels[l];
  // level vectors: b (l >= 1), y, d, xa, xb  (level 0's b and final x are the caller's r and z)
  size_t tot = 0;
  for (int l = 0; l < n_levels; ++l) tot += 5 * (size_t)((levels[l].A.n_cols > levels[l].n_rows ? levels[l].A.n_cols : levels[l].n_rows) + 64);
  if (hipMalloc(&mg->mem, tot * sizeof(double)) != hipSuccess) {
    delete mg;
    OX_FAIL("ox_mg_create: hipMalloc of %zu bytes failed", tot * sizeof(double));
  }
  OX_HIP(hipMemset(mg->mem, 0, tot * sizeof(double)));
  double *vb[OX_MG_MAX_LEVELS], *vy[OX_MG_MAX_LEVELS], *vd[OX_MG_MAX_LEVELS], *vx[OX_MG_MAX_LEVELS][2];
  {
    double *p = static_cast<double *>(mg->mem);
    for (int l = 0; l < n_levels; ++l) {
      const size_t m = (size_t)((levels[l].A.n_cols > levels[l].n_rows ? levels[l].A.n_cols : levels[l].n_rows) + 64);
      vb[l] = p, vy[l] = p + m, vd[l] = p + 2 * m, vx[l][0] = p + 3 * m, vx[l][1] = p + 4 * m;
      p += 5 * m;
    }
    vb[0] = MG_B0;
  }
  // first level that runs in the tail (the coarse solve always does)
  int lt = c;
  for (int l = 0; l < c; ++l)
    if (levels[l].n_rows <= T) {
      lt = l;
      break;
    }
  std::vector<MgPhase> tail;
  bool tail_op = false;
  auto emit = [&](const MgPhase &p) {
    if (p.level >= lt) {
      if (!tail_op) {
        MgOp o{};
        o.kind = OP_TAIL;
        mg->ops.push_back(o);
        tail_op = true;
      }
      tail.push_back(p);
    } else {
      MgOp o{};
      o.kind = OP_PHASE;
      o.ph = p;
      mg->ops.push_back(o);
    }
  };
  // a Chebyshev step on level l: on a grid level 0, the caller's mat-vec then MG_STEPY
  auto step = [&](int l, int j, const double *xin, double *xo) {
    const ox_mg_level &L = levels[l];
    MgPhase p{};
    p.level = l;
    p.n = L.n_rows;
    p.M = mg_mat(L.A);
    p.dinv = L.dinv;
    p.b = vb[l];
    p.xin = xin;
    p.xout = xo;
    p.d = vd[l];
    p.cd = L.cheb[2 * j];
    p.cr = L.cheb[2 * j + 1];
    if (l == 0 && lt > 0) {
      MgOp o{};
      o.kind = OP_SPMV0;
      o.x = const_cast<double *>(xin);
      o.y = vy[0];
      mg->ops.push_back(o);
      p.kind = MG_STEPY;
      p.y = vy[0];
    } else {
      p.kind = MG_STEP;
    }
    emit(p);
  };
  int cur[OX_MG_MAX_LEVELS];
  if (c == 0) {  // one level: the dense solve
    MgPhase p{};
    p.kind = MG_COARSE;
    p.level = 0;
    p.n = levels[0].n_rows;
    p.M.vals = coarse_inv;
    p.b = MG_B0;
    p.out = MG_Z0;
    emit(p);
  } else {
    // (MG_COARSE reads b directly: level 0 never is the coarsest here)
    {
      MgPhase p{};
      p.kind = MG_S0;
      p.level = 0;
      p.n = levels[0].n_rows;
      p.dinv = levels[0].dinv;
      p.b = vb[0];
      p.d = vd[0];
      p.xout = vx[0][0];
      p.cr = levels[0].cheb[1];
      emit(p);
    }
    for (int l = 0; l < c; ++l) {
      const ox_mg_level &L = levels[l];
      int k = 0;  // x of level l in vx[l][k]
      for (int j = 1; j < L.degree; ++j) {
        step(l, j, vx[l][k], vx[l][1 - k]);
        k = 1 - k;
      }
      cur[l] = k;
      // y = A x
      if (l == 0 && lt > 0) {
        MgOp o{};
        o.kind = OP_SPMV0;
        o.x = vx[0][k];
        o.y = vy[0];
        mg->ops.push_back(o);
      } else {
        MgPhase p{};
        p.kind = MG_SPMV;
        p.level = l;
        p.n = L.n_rows;
        p.M = mg_mat(L.A);
        p.xin = vx[l][k];
        p.out = vy[l];
        emit(p);
      }
      // b_{l+1} = R (b - y), with the first smoothing step of level l+1
      MgPhase p{};
      p.kind = MG_RESTRICT;
      p.level = l;
      p.n = levels[l + 1].n_rows;
      p.M = mg_mat(L.R);
      p.b = vb[l];
      p.y = vy[l];
      p.out = vb[l + 1];
      if (l + 1 < c) {
        p.dinv2 = levels[l + 1].dinv;
        p.d2 = vd[l + 1];
        p.x2 = vx[l + 1][0];
        p.cr2 = levels[l + 1].cheb[1];
      }
      // (a restriction into the tail's first level reads level l's vectors: it belongs to level l, a grid phase when
      // l < lt)
      emit(p);
    }
    {
      MgPhase p{};
      p.kind = MG_COARSE;
      p.level = c;
      p.n = levels[c].n_rows;
      p.M.vals = coarse_inv;
      p.b = vb[c];
      p.out = vx[c][0];
      emit(p);
      cur[c] = 0;
    }
    for (int l = c - 1; l >= 0; --l) {
      const ox_mg_level &L = levels[l];
      int k = cur[l];
      MgPhase p{};
      p.kind = MG_PROLONG;
      p.level = l;
      p.n = L.n_rows;
      p.M = mg_mat(L.P);
      p.xin = vx[l][k];
      p.xc = vx[l + 1][cur[l + 1]];
      p.xout = (l == 0 && L.degree == 0) ? MG_Z0 : vx[l][1 - k];
      emit(p);
      k = 1 - k;
      for (int j = 0; j < L.degree; ++j) {
        double *xo = (l == 0 && j + 1 == L.degree) ? MG_Z0 : vx[l][1 - k];
        step(l, j, vx[l][k], xo);
        k = 1 - k;
      }
      cur[l] = k;
    }
  }
  mg->n_tail = (int)tail.size();
  mg->tail_dev = nullptr;
  if (!tail.empty()) {
    if (hipMalloc(&mg->tail_dev, tail.size() * sizeof(MgPhase)) != hipSuccess) {
      (void)hipFree(mg->mem);
      delete mg;
      OX_FAIL("ox_mg_create: hipMalloc of the tail's phases failed");
    }
    OX_HIP(hipMemcpy(mg->tail_dev, tail.data(), tail.size() * sizeof(MgPhase), hipMemcpyHostToDevice));
  }
  mg->kernels = (int)mg->ops.size();
  *out = mg;
  return 0;
}

extern "C" int ox_mg_destroy(ox_mg *mg) {
  if (!mg) return 0;
  if (mg->tail_dev) (void)hipFree(mg->tail_dev);
  if (mg->mem) (void)hipFree(mg->mem);
  delete mg;
  return 0;
}

extern "C" int ox_mg_kernels_per_cycle(const ox_mg *mg) { return mg ? mg->kernels : -1; }
int64_t ox_mg_fine_rows(const ox_mg *mg) { return mg ? mg->lv[0].n_rows : -1; }

// z = B r on `st`; every kernel is a no-op once *done (nullptr: always runs).  (Used by OX_KSP_CG_MG: ox_ksp.hip.)
int ox_mg_vcycle(const ox_mg *mg, const double *r, double *z, const int *done, hipStream_t st) {
  const ox_sell *A0 = &mg->lv[0].A;
  for (const MgOp &o : mg->ops) {
    if (o.kind == OP_SPMV0) {
      if (ox_spmv_dist(A0, o.x, o.y, 1, OX_EPI_NONE, nullptr, nullptr, nullptr, done, nullptr, st)) return -1;
    } else if (o.kind == OP_TAIL) {
      hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(OX_MG_TAIL_T), 0, st, mg->tail_dev, mg->n_tail, r, z, done);
      OX_LAUNCH_CHECK();
    } else {
      const int64_t nb = (o.ph.n + 255) / 256;
      hipLaunchKernelGGL(k_mg_phase, dim3((unsigned)nb), dim3(256), 0, st, o.ph, r, z, done);
      OX_LAUNCH_CHECK();
    }
  }
  return 0;
}

extern "C" int ox_mg_apply(const ox_mg *mg, const double *r, double *z, void *stream) {
  if (!mg || !r || !z) OX_FAIL("ox_mg_apply: null argument");
  return ox_mg_vcycle(mg, r, z, nullptr, ox_stream(stream));
}
