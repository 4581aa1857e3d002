// translation unit: gemm5 kernels with the per-row-multiplier epilogue (EPI_GENERIC_ROWMUL, fp16 operands): the gated residual projections
// of f5hip_cfm_sample_grids, where the rows of one launch sit at different time points
#include "gemm5.h"
#include "gemm_launch.h"

hipError_t f5_launch_gemm5_rowmul(const GemmArgs& a, int rb, int cb, int n_pad, hipStream_t st) {
    return launch_gemm5<true, EPI_GENERIC_ROWMUL>(a, rb, cb, n_pad, st);
}
