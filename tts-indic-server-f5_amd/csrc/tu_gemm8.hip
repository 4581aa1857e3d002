// translation unit: gemm8 (gemm8.h), the MXFP8 block GEMM of gemm_planes == 4, and the weight quantiser that feeds it
#include "gemm8.h"
#include "gemm_launch.h"

hipError_t f5_launch_gemm8(int epi, const GemmArgs& a, const unsigned char* w8, const unsigned int* s8, int n_pad, hipStream_t st) {
    if (!w8 || !s8 || !gemm8_covers(epi, a.K, n_pad)) return hipErrorInvalidValue;
    const bool wide = n_pad % 256 == 0;   // 64 x 256 tiles where they divide N: one conversion of the A rows serves 16 MFMAs instead of 8
    if (epi == EPI_GENERIC_ROWMUL) return wide ? launch_gemm8_t<EPI_GENERIC_ROWMUL, 16>(a, w8, s8, n_pad, st) : launch_gemm8_t<EPI_GENERIC_ROWMUL, 8>(a, w8, s8, n_pad, st);
    return wide ? launch_gemm8_t<EPI_GENERIC, 16>(a, w8, s8, n_pad, st) : launch_gemm8_t<EPI_GENERIC, 8>(a, w8, s8, n_pad, st);
}

hipError_t f5_launch_quant_w8(const float* w, int N, int n_pad, int K, int ldw, unsigned char* w8, unsigned int* s8, hipStream_t st) {
    if (!w || !w8 || !s8 || N <= 0 || n_pad % 16 || N > n_pad || K <= 0 || K % 128 || ldw < K || ldw % 4) return hipErrorInvalidValue;
    const long long blocks = (long long)n_pad * (K / 32);
    hipLaunchKernelGGL(quant_w8_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, w, N, n_pad, K, ldw, w8, reinterpret_cast<unsigned char*>(s8));
    return hipGetLastError();
}
