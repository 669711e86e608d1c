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
#include "ox_common.h"

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
