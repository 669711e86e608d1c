// Fischer's projected initial guesses (PETSc's KSPGUESSFISCHER, -ksp_guess_type fischer; P. Fischer, CMAME 163, 1998) for
// CG solves that repeat on one operator with changing right-hand sides.
//
// Per column c of an interleaved (n x nc) block the object keeps k <= size A-orthonormal directions x~_j (x~_i' A x~_j =
// delta_ij), stored UNSCALED as v_j with a per-(slot, column) scale sigma_j: x~_j = sigma_j v_j (model 1 also keeps
// w_j = A v_j, so b~_j = sigma_j w_j).  A slot whose direction was rejected (the skip rule) has sigma = 0: it acts as a
// zero vector.  Every coefficient below is sigma_j^2 times a raw sum v_j . y, formed on the device from the reduced sums:
//   form     x0 = x_w + sum_j x~_j (x~_j . (b - A x_w))        (all local rows; model 1: A x0 as well, owned rows)
//   update   d = x - x0;  d -= sum_j x~_j (x~_j . A d);  sigma_k = 1 / sqrt(d . A d)  (model 1: A d by the same recurrence)
// The slot vectors are tall-skinny streams: every kernel reads them once with 16-B loads (ox_flat_pairs of ox_ksp.hip).
// Dot products run over the owned rows, per block in a fixed order and then over the blocks in a fixed order (one block
// per sum): identical runs give identical bits.  The host reads nothing between form, solve and update.
#include "ox_kernels.h"

#define OX_GUESS_MAX 32  // slots: the storage and register budget of this path (PETSc has no such limit)
#define OX_GUESS_J 8     // slots per block row of k_guess_dots: J * NC accumulators per thread
#define OX_GUESS_CHUNKS ((OX_GUESS_MAX + 1 + OX_GUESS_J - 1) / OX_GUESS_J)

struct GuessPtrs {
  const double *p[OX_GUESS_MAX + 1];
};

struct ox_guess {
  int64_t n_rows, n_owned;  // local rows (owned + ghost) and owned rows
  int nc, model, size, k;
  int formed;               // ox_guess_form wrote x0 into v[k] (the update's d = x - x0)
  void *mem;
  double *v[OX_GUESS_MAX];  // [n_rows * nc] directions (unscaled)
  double *w[OX_GUESS_MAX];  // model 1: [n_owned * nc] A v_j
  double *y;                // [n_owned * nc] scratch: A x_w, A x0 after a full basis, model 2's A d
  double *sigma;            // [OX_GUESS_MAX * nc]
  double *sums;             // [(OX_GUESS_MAX + 1) * nc] raw sums, then [nc] d . A d after orthogonalisation
  double *partial;          // [OX_GUESS_CHUNKS][OX_VEC_MAX_BLOCKS][OX_GUESS_J * nc]
};

// ---------------------------------------------------------------------------------------------------------------------
// kernels (flat traversal helpers as in ox_ksp.hip: two consecutive elements per thread, 16-B loads)
template <int NC, class F>
__device__ __forceinline__ void guess_pairs(int64_t n, F &&f) {
  const int64_t tot = n * NC, n2 = tot >> 1;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += stride) {
    const int64_t e = 2 * i;
    const int c0 = (int)(e % NC);
    f(e, c0, c0 + 1 == NC ? 0 : c0 + 1, true);
  }
  if ((tot & 1) && blockIdx.x == 0 && threadIdx.x == 0) f(tot - 1, (int)((tot - 1) % NC), 0, false);
}
// elements [e0, e1) one by one (the ghost rows: a halo is small against the owned block)
template <int NC, class F>
__device__ __forceinline__ void guess_tail(int64_t e0, int64_t e1, F &&f) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = e0 + (int64_t)blockIdx.x * 256 + threadIdx.x; e < e1; e += stride) f(e, (int)(e % NC));
}
__device__ __forceinline__ double2 g_ld2(const double *p, int64_t e, bool two) {
  if (two) return *reinterpret_cast<const double2 *>(p + e);
  return make_double2(p[e], 0.0);
}
__device__ __forceinline__ void g_st2(double *p, int64_t e, double2 v, bool two) {
  if (two) *reinterpret_cast<double2 *>(p + e) = v;
  else p[e] = v.x;
}
template <int NC, int NV>
__device__ __forceinline__ void g_acc(double (&s)[NV], int off, int c, double a, double b) {
#pragma unroll
  for (int q = 0; q < NC; ++q) s[off + q] = (c == q) ? fma(a, b, s[off + q]) : s[off + q];
}
// coefficients sigma_j^2 * raw_j of slots j < k into LDS
template <int NC>
__device__ __forceinline__ void guess_coef(double *a, int k, const double *raw, const double *sigma) {
  for (int i = threadIdx.x; i < k * NC; i += blockDim.x) {
    const double s = sigma[i];
    a[i] = s * s * raw[i];
  }
  __syncthreads();
}

// partial[(chunk * nblk + block) * J*NC + j*NC + c] = sum over the owned rows of V_{chunk*J + j}[e] * (y[e] - z[e]), z may be
// nullptr; grid (nblk, chunks)
template <int NC>
__global__ __launch_bounds__(256) void k_guess_dots(int64_t n, const double *__restrict__ y, const double *__restrict__ z,
                                                    GuessPtrs V, int nv, double *__restrict__ partial) {
  constexpr int NV = OX_GUESS_J * NC;
  __shared__ double red[4 * NV];
  const int j0 = blockIdx.y * OX_GUESS_J;
  const int nj = min(OX_GUESS_J, nv - j0);
  const double *vp[OX_GUESS_J];
#pragma unroll
  for (int j = 0; j < OX_GUESS_J; ++j) vp[j] = j < nj ? V.p[j0 + j] : nullptr;
  double s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = 0.0;
  guess_pairs<NC>(n, [&](int64_t e, int ca, int cb, bool two) {
    double2 r = g_ld2(y, e, two);
    if (z) {
      const double2 q = g_ld2(z, e, two);
      r.x -= q.x;
      r.y -= q.y;
    }
#pragma unroll
    for (int j = 0; j < OX_GUESS_J; ++j) {
      if (j < nj) {
        const double2 v = g_ld2(vp[j], e, two);
        g_acc<NC>(s, j * NC, ca, v.x, r.x);
        if (two) g_acc<NC>(s, j * NC, cb, v.y, r.y);
      }
    }
  });
  ox_block_sum_256<NV>(s, red);
  if (threadIdx.x == 0) {
    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) out[i] = s[i];
  }
}

// sums[chunk * J*NC + i] = sum over the blocks of partial[chunk][block][i], blocks in order; one block per sum, grid
// (J*NC, chunks); only the first `nsum` sums are written
__global__ __launch_bounds__(256) void k_guess_reduce(const double *__restrict__ partial, int nblk, int nvb, int nsum,
                                                      double *__restrict__ sums) {
  __shared__ double red[4];
  const int i = blockIdx.x, chunk = blockIdx.y;
  const int o = chunk * nvb + i;
  if (o >= nsum) return;
  const double *p = partial + (size_t)chunk * nblk * nvb + i;
  double s[1] = {0.0};
  for (int b = threadIdx.x; b < nblk; b += 256) s[0] += p[(size_t)b * nvb];
  ox_block_sum_256<1>(s, red);
  if (threadIdx.x == 0) sums[o] = s[0];
}

// x0 = x_w + sum_{j<k} a_j v_j on all local rows (x_w = 0 unless xw); copy: the same into v[k] (nullptr: none);
// model 1 (W, ax0 != nullptr): ax0 = A x_w + sum_j a_j w_j on the owned rows (axw == nullptr: A x_w = 0)
template <int NC>
__global__ __launch_bounds__(256) void k_guess_combine(int64_t n, int64_t n_owned, int k, const double *raw,
                                                       const double *sigma, GuessPtrs V, GuessPtrs W, double *x, int xw,
                                                       double *copy, const double *axw, double *ax0) {
  __shared__ double a[OX_GUESS_MAX * NC];
  guess_coef<NC>(a, k, raw, sigma);
  guess_pairs<NC>(n_owned, [&](int64_t e, int ca, int cb, bool two) {
    double2 s = xw ? g_ld2(x, e, two) : make_double2(0.0, 0.0);
    for (int j = 0; j < k; ++j) {
      const double2 v = g_ld2(V.p[j], e, two);
      s.x = fma(a[j * NC + ca], v.x, s.x);
      s.y = fma(a[j * NC + cb], v.y, s.y);
    }
    g_st2(x, e, s, two);
    if (copy) g_st2(copy, e, s, two);
    if (ax0) {
      double2 t = axw ? g_ld2(axw, e, two) : make_double2(0.0, 0.0);
      for (int j = 0; j < k; ++j) {
        const double2 w = g_ld2(W.p[j], e, two);
        t.x = fma(a[j * NC + ca], w.x, t.x);
        t.y = fma(a[j * NC + cb], w.y, t.y);
      }
      g_st2(ax0, e, t, two);
    }
  });
  guess_tail<NC>(n_owned * NC, n * NC, [&](int64_t e, int c) {
    double s = xw ? x[e] : 0.0;
    for (int j = 0; j < k; ++j) s = fma(a[j * NC + c], V.p[j][e], s);
    x[e] = s;
    if (copy) copy[e] = s;
  });
}

// d = x - d (sub) or d = x, all local rows
template <int NC>
__global__ __launch_bounds__(256) void k_guess_sub(int64_t n, const double *__restrict__ x, double *d, int sub) {
  guess_pairs<NC>(n, [&](int64_t e, int, int, bool two) {
    double2 r = g_ld2(x, e, two);
    if (sub) {
      const double2 q = g_ld2(d, e, two);
      r.x -= q.x;
      r.y -= q.y;
    }
    g_st2(d, e, r, two);
  });
}

// d -= sum_{j<k} c_j v_j on all local rows; model 1 (ad != nullptr): ad -= sum_j c_j w_j on the owned rows and
// partial[block][c] = d . ad over them
template <int NC>
__global__ __launch_bounds__(256) void k_guess_orth(int64_t n, int64_t n_owned, int k, const double *raw,
                                                    const double *sigma, GuessPtrs V, GuessPtrs W, double *d, double *ad,
                                                    double *__restrict__ partial) {
  __shared__ double a[OX_GUESS_MAX * NC];
  __shared__ double red[4 * NC];
  guess_coef<NC>(a, k, raw, sigma);
  double s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  guess_pairs<NC>(n_owned, [&](int64_t e, int ca, int cb, bool two) {
    double2 dd = g_ld2(d, e, two);
    for (int j = 0; j < k; ++j) {
      const double2 v = g_ld2(V.p[j], e, two);
      dd.x = fma(-a[j * NC + ca], v.x, dd.x);
      dd.y = fma(-a[j * NC + cb], v.y, dd.y);
    }
    g_st2(d, e, dd, two);
    if (ad) {
      double2 t = g_ld2(ad, e, two);
      for (int j = 0; j < k; ++j) {
        const double2 w = g_ld2(W.p[j], e, two);
        t.x = fma(-a[j * NC + ca], w.x, t.x);
        t.y = fma(-a[j * NC + cb], w.y, t.y);
      }
      g_st2(ad, e, t, two);
      g_acc<NC>(s, 0, ca, dd.x, t.x);
      if (two) g_acc<NC>(s, 0, cb, dd.y, t.y);
    }
  });
  guess_tail<NC>(n_owned * NC, n * NC, [&](int64_t e, int c) {
    double dd = d[e];
    for (int j = 0; j < k; ++j) dd = fma(-a[j * NC + c], V.p[j][e], dd);
    d[e] = dd;
  });
  if (partial) {
    ox_block_sum_256<NC>(s, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) partial[(size_t)blockIdx.x * NC + c] = s[c];
    }
  }
}

// One wave: sigma_k = 1 / sqrt(post) per column, or 0 (the skip rule) when post <= 1e-20 pre or either is <= 0.
__global__ __launch_bounds__(64) void k_guess_scale(int nc, const double *pre, const double *post, double *sigma) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  const double p = pre[c], q = post[c];
  sigma[c] = (p > 0.0 && q > 0.0 && q > 1e-20 * p) ? 1.0 / sqrt(q) : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
static int guess_allreduce(const ox_dist *dist, double *buf, int n, hipStream_t st) {
  if (!dist) return 0;
  // (the xGMI-window transport reduces at most OX_MAX_NV values per call)
  const int step = dist->p2p ? OX_MAX_NV : n;
  for (int o = 0; o < n; o += step)
    if (ox_allreduce_impl(dist, buf + o, n - o < step ? n - o : step, st)) return -1;
  return 0;
}

// sums[0 .. nv*nc) = V_j . (y - z) over the owned rows, all-reduced
static int guess_dots(const ox_guess *g, const double *y, const double *z, const GuessPtrs &V, int nv, double *sums,
                      const ox_dist *dist, hipStream_t st) {
  const int nblk = ox_vec_blocks(g->n_owned * g->nc);
  const int chunks = (nv + OX_GUESS_J - 1) / OX_GUESS_J;
  const dim3 grid(nblk, chunks);
  switch (g->nc) {
    case 1: hipLaunchKernelGGL(k_guess_dots<1>, grid, dim3(256), 0, st, g->n_owned, y, z, V, nv, g->partial); break;
    case 2: hipLaunchKernelGGL(k_guess_dots<2>, grid, dim3(256), 0, st, g->n_owned, y, z, V, nv, g->partial); break;
    default: hipLaunchKernelGGL(k_guess_dots<3>, grid, dim3(256), 0, st, g->n_owned, y, z, V, nv, g->partial); break;
  }
  OX_LAUNCH_CHECK();
  const int nvb = OX_GUESS_J * g->nc;
  hipLaunchKernelGGL(k_guess_reduce, dim3(nvb, chunks), dim3(256), 0, st, g->partial, nblk, nvb, nv * g->nc, sums);
  OX_LAUNCH_CHECK();
  return guess_allreduce(dist, sums, nv * g->nc, st);
}

static GuessPtrs guess_ptrs(double *const *p, int k, const double *extra) {
  GuessPtrs P{};
  for (int j = 0; j < k; ++j) P.p[j] = p[j];
  P.p[k] = extra;
  return P;
}

extern "C" int ox_guess_create(int64_t n_rows, int64_t n_owned, int ncomp, int model, int size, ox_guess **out) {
  if (!out) OX_FAIL("ox_guess_create: null argument");
  *out = nullptr;
  if (ncomp < 1 || ncomp > OX_MAXC) OX_FAIL("ox_guess_create: ncomp=%d", ncomp);
  if (model != 1 && model != 2) OX_FAIL("ox_guess_create: model %d (1 or 2)", model);
  if (size < 1 || size > OX_GUESS_MAX) OX_FAIL("ox_guess_create: size %d (1..%d)", size, OX_GUESS_MAX);
  if (n_owned < 0 || n_rows < n_owned) OX_FAIL("ox_guess_create: %lld rows, %lld owned", (long long)n_rows, (long long)n_owned);
  auto al = [](size_t d) { return (d + 31) & ~(size_t)31; };  // doubles, 256-B aligned slices
  const size_t sv = al((size_t)n_rows * ncomp), so = al((size_t)n_owned * ncomp);
  const size_t ssig = al((size_t)OX_GUESS_MAX * ncomp), ssum = al((size_t)(OX_GUESS_MAX + 2) * ncomp);
  const size_t spart = (size_t)OX_GUESS_CHUNKS * OX_VEC_MAX_BLOCKS * OX_GUESS_J * ncomp;
  const size_t tot = sv * size + (model == 1 ? so * size : 0) + so + ssig + ssum + spart;
  ox_guess *g = new ox_guess();
  g->n_rows = n_rows, g->n_owned = n_owned, g->nc = ncomp, g->model = model, g->size = size;
  if (hipMalloc(&g->mem, tot * sizeof(double)) != hipSuccess) {
    delete g;
    OX_FAIL("ox_guess_create: hipMalloc of %zu bytes failed", tot * sizeof(double));
  }
  double *p = static_cast<double *>(g->mem);
  for (int j = 0; j < size; ++j, p += sv) g->v[j] = p;
  if (model == 1)
    for (int j = 0; j < size; ++j, p += so) g->w[j] = p;
  g->y = p, p += so;
  g->sigma = p, p += ssig;
  g->sums = p, p += ssum;
  g->partial = p;
  // (zero slots and scales: a slot's ghost rows and padding are defined before its first use)
  if (hipMemset(g->mem, 0, tot * sizeof(double)) != hipSuccess) {
    (void)hipFree(g->mem);
    delete g;
    OX_FAIL("ox_guess_create: hipMemset failed");
  }
  *out = g;
  return 0;
}

extern "C" int ox_guess_destroy(ox_guess *g) {
  if (!g) return 0;
  OX_HIP(hipFree(g->mem));
  delete g;
  return 0;
}

extern "C" int ox_guess_reset(ox_guess *g) {
  if (!g) OX_FAIL("ox_guess_reset: null handle");
  g->k = 0;
  g->formed = 0;
  return 0;
}

extern "C" int ox_guess_dim(const ox_guess *g) { return g ? g->k : -1; }

extern "C" size_t ox_guess_bytes(const ox_guess *g) {
  if (!g) return 0;
  return sizeof(double) * ((size_t)g->n_rows * g->nc * g->size + (g->model == 1 ? (size_t)g->n_owned * g->nc * g->size : 0));
}

extern "C" int ox_guess_form(ox_guess *g, const ox_sell *A, const double *b, double *x, int nonzero_guess, const double *ax_w,
                             const double **ax0_out, const ox_dist *dist, void *stream) {
  if (!g || !A || !b || !x || !ax0_out) OX_FAIL("ox_guess_form: null argument");
  if (A->n_rows != g->n_owned || A->n_cols != g->n_rows)
    OX_FAIL("ox_guess_form: operator %lld x %lld, basis of %lld x %lld rows", (long long)A->n_rows, (long long)A->n_cols,
            (long long)g->n_owned, (long long)g->n_rows);
  *ax0_out = nullptr;
  g->formed = 0;
  if (g->k == 0) return 0;  // the caller's solve, as it stands
  hipStream_t st = ox_stream(stream);
  const int k = g->k, nc = g->nc;
  const double *axw = nullptr;
  if (nonzero_guess) {
    axw = ax_w;
    if (!axw) {
      if (ox_spmv_dist(A, x, g->y, nc, OX_EPI_NONE, nullptr, nullptr, nullptr, nullptr, dist, st)) return -1;
      axw = g->y;
    }
  }
  if (guess_dots(g, b, axw, guess_ptrs(g->v, k, nullptr), k, g->sums, dist, st)) return -1;
  double *copy = k < g->size ? g->v[k] : nullptr;
  double *ax0 = g->model == 1 ? (k < g->size ? g->w[k] : g->y) : nullptr;
  const GuessPtrs V = guess_ptrs(g->v, k, nullptr);
  const GuessPtrs W = g->model == 1 ? guess_ptrs(g->w, k, nullptr) : GuessPtrs{};
  const int nblk = ox_vec_blocks(g->n_rows * nc);
  switch (nc) {
    case 1: hipLaunchKernelGGL(k_guess_combine<1>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, x, nonzero_guess, copy, axw, ax0); break;
    case 2: hipLaunchKernelGGL(k_guess_combine<2>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, x, nonzero_guess, copy, axw, ax0); break;
    default: hipLaunchKernelGGL(k_guess_combine<3>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, x, nonzero_guess, copy, axw, ax0); break;
  }
  OX_LAUNCH_CHECK();
  g->formed = copy != nullptr;
  *ax0_out = ax0;
  return 0;
}

extern "C" int ox_guess_update(ox_guess *g, const ox_sell *A, const double *x, const ox_dist *dist, void *stream) {
  if (!g || !A || !x) OX_FAIL("ox_guess_update: null argument");
  if (A->n_rows != g->n_owned || A->n_cols != g->n_rows)
    OX_FAIL("ox_guess_update: operator %lld x %lld, basis of %lld x %lld rows", (long long)A->n_rows, (long long)A->n_cols,
            (long long)g->n_owned, (long long)g->n_rows);
  hipStream_t st = ox_stream(stream);
  const int nc = g->nc;
  int sub = g->formed && g->k > 0 && g->k < g->size;
  if (g->k == g->size) g->k = 0;  // restart: the latest solution alone
  const int k = g->k;
  g->formed = 0;
  double *d = g->v[k];
  double *ad = g->model == 1 ? g->w[k] : g->y;
  const int nblk = ox_vec_blocks(g->n_rows * nc);
  switch (nc) {
    case 1: hipLaunchKernelGGL(k_guess_sub<1>, dim3(nblk), dim3(256), 0, st, g->n_rows, x, d, sub); break;
    case 2: hipLaunchKernelGGL(k_guess_sub<2>, dim3(nblk), dim3(256), 0, st, g->n_rows, x, d, sub); break;
    default: hipLaunchKernelGGL(k_guess_sub<3>, dim3(nblk), dim3(256), 0, st, g->n_rows, x, d, sub); break;
  }
  OX_LAUNCH_CHECK();
  if (ox_spmv_dist(A, d, ad, nc, OX_EPI_NONE, nullptr, nullptr, nullptr, nullptr, dist, st)) return -1;
  // beta_j (raw) for j < k and d . A d before the orthogonalisation: one pass
  double *pre = g->sums + (size_t)k * nc, *post = g->sums + (size_t)(OX_GUESS_MAX + 1) * nc;
  if (guess_dots(g, ad, nullptr, guess_ptrs(g->v, k, d), k + 1, g->sums, dist, st)) return -1;
  if (k == 0) {
    post = pre;
  } else {
    const GuessPtrs V = guess_ptrs(g->v, k, nullptr);
    const GuessPtrs W = g->model == 1 ? guess_ptrs(g->w, k, nullptr) : GuessPtrs{};
    double *fused = g->model == 1 ? ad : nullptr;
    double *part = g->model == 1 ? g->partial : nullptr;
    switch (nc) {
      case 1: hipLaunchKernelGGL(k_guess_orth<1>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, d, fused, part); break;
      case 2: hipLaunchKernelGGL(k_guess_orth<2>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, d, fused, part); break;
      default: hipLaunchKernelGGL(k_guess_orth<3>, dim3(nblk), dim3(256), 0, st, g->n_rows, g->n_owned, k, g->sums, g->sigma, V, W, d, fused, part); break;
    }
    OX_LAUNCH_CHECK();
    if (g->model == 1) {
      hipLaunchKernelGGL(k_guess_reduce, dim3(nc, 1), dim3(256), 0, st, g->partial, nblk, nc, nc, post);
      OX_LAUNCH_CHECK();
      if (guess_allreduce(dist, post, nc, st)) return -1;
    } else {  // model 2 keeps no A v_j: A d once more
      if (ox_spmv_dist(A, d, ad, nc, OX_EPI_NONE, nullptr, nullptr, nullptr, nullptr, dist, st)) return -1;
      if (guess_dots(g, ad, nullptr, guess_ptrs(g->v, 0, d), 1, post, dist, st)) return -1;
    }
  }
  hipLaunchKernelGGL(k_guess_scale, dim3(1), dim3(64), 0, st, nc, pre, post, g->sigma + (size_t)k * nc);
  OX_LAUNCH_CHECK();
  g->k = k + 1;
  return 0;
}
