// group_impl.hpp — the __global__ kernels and launchers of the column-group linear map (groupops.hpp) for one limb count.
// Included by kern_grp_nl*.hip with BGN_NL defined: units of their own, so that the table and walk kernels compile beside
// the kern_nl*.hip units instead of lengthening them.  kernels_impl.hpp declares the launchers and puts them into the
// limb count's KernelTable.
#pragma once
#include "groupops.hpp"

namespace bgn {

#define BGN_GRP_CAT2(a, b) a##b
#define BGN_GRP_CAT(a, b) BGN_GRP_CAT2(a, b)
#define BGN_GRP_FN(name) BGN_GRP_CAT(BGN_GRP_CAT(name, _nl), BGN_NL)

constexpr int GNL_ = BGN_NL;

static inline unsigned grp_grid_for(size_t count) { return (unsigned)((count + FP_BLOCK - 1) / FP_BLOCK); }

template <int NL>
__global__ void __launch_bounds__(FP_BLOCK)
k_grp_codes(GrpCodesArgs A) {
  const size_t i = (size_t)blockIdx.x * FP_BLOCK + threadIdx.x;
  if (i < A.ngroups * A.nrows) grp_codes_lane(A, i);
}

template <int NL, int LEVEL>
__global__ void __launch_bounds__(FP_BLOCK)
k_grp_table(const FpParams<NL>* __restrict__ P, const PairingConsts* __restrict__ C, GrpTableArgs A) {
  __shared__ LFp<NL> L[4];
  const size_t nq = A.nvec * A.ngroups;
  size_t q = (size_t)blockIdx.x * FP_BLOCK + threadIdx.x;
  const bool live = q < nq;
  if (!__ballot(live)) return;
  if (!live) q = nq - 1;                     // keep every index in range; nothing but the lane's own scratch is stored
  if (LEVEL == 1)
    grp_table_g1_lane<NL>(A, q, live, (size_t)gridDim.x * FP_BLOCK, L, C, P);
  else
    grp_table_gt_lane<NL>(A, q, live, L, P);
}

template <int NL, int LEVEL>
__global__ void __launch_bounds__(FP_BLOCK)
k_grp_walk(const FpParams<NL>* __restrict__ P, const PairingConsts* __restrict__ C, GrpWalkArgs A) {
  __shared__ LFp<NL> L[4];
  const size_t total = A.nvec * A.nchunk * A.nrows;
  size_t lane = (size_t)blockIdx.x * FP_BLOCK + threadIdx.x;
  const bool live = lane < total;
  if (!__ballot(live)) return;
  if (!live) lane = total - 1;               // keep every index in range; nothing is taken or stored
  if (LEVEL == 1)
    grp_walk_g1_lane<NL>(A, lane, live, L, C, P);
  else
    grp_walk_gt_lane<NL>(A, lane, live, L, P);
}

void BGN_GRP_FN(launch_grp_codes)(hipStream_t s, GrpCodesArgs a) {
  if (!a.nrows || !a.ngroups) return;
  hipLaunchKernelGGL(k_grp_codes<GNL_>, dim3(grp_grid_for(a.ngroups * a.nrows)), dim3(FP_BLOCK), 0, s, a);
}

void BGN_GRP_FN(launch_grp_table)(hipStream_t s, const void* params, const PairingConsts* consts, int level, GrpTableArgs a) {
  const size_t nq = a.nvec * a.ngroups;
  if (!nq) return;
  if (level == 1)
    hipLaunchKernelGGL((k_grp_table<GNL_, 1>), dim3(grp_grid_for(nq)), dim3(FP_BLOCK), 0, s, (const FpParams<GNL_>*)params,
                       consts, a);
  else
    hipLaunchKernelGGL((k_grp_table<GNL_, 2>), dim3(grp_grid_for(nq)), dim3(FP_BLOCK), 0, s, (const FpParams<GNL_>*)params,
                       consts, a);
}

void BGN_GRP_FN(launch_grp_walk)(hipStream_t s, const void* params, const PairingConsts* consts, int level, GrpWalkArgs a) {
  const size_t total = a.nvec * a.nchunk * a.nrows;
  if (!total || !a.ngroups) return;
  if (level == 1)
    hipLaunchKernelGGL((k_grp_walk<GNL_, 1>), dim3(grp_grid_for(total)), dim3(FP_BLOCK), 0, s, (const FpParams<GNL_>*)params,
                       consts, a);
  else
    hipLaunchKernelGGL((k_grp_walk<GNL_, 2>), dim3(grp_grid_for(total)), dim3(FP_BLOCK), 0, s, (const FpParams<GNL_>*)params,
                       consts, a);
}

// Host-side handle of kernel `which` (bgn_last_kernel_resources): 0, 1 the walk of level 1, 2; 2, 3 the table kernel.
const void* BGN_GRP_FN(grp_kernel)(int which) {
  return which == 0 ? (const void*)k_grp_walk<GNL_, 1> : which == 1 ? (const void*)k_grp_walk<GNL_, 2>
       : which == 2 ? (const void*)k_grp_table<GNL_, 1> : (const void*)k_grp_table<GNL_, 2>;
}

}  // namespace bgn
