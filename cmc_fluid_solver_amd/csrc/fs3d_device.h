// Device primitives shared by the sweep kernels (kernels_pipe.hip, kernels_part.hip): the compile-time loop, raw buffer access
// and the refined fp32 reciprocal.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

// Compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>).  Loops over register arrays that are too
// large for `#pragma unroll` (the unroller gives up past its size threshold, the cell indices of the register arrays turn dynamic
// and the arrays land in scratch memory): instantiate them instead.
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// Raw buffer access: address = descriptor base (4 SGPRs) + soffset (1 SGPR, wave-uniform row) +
// voffset (1 VGPR, per-lane byte offset).  One SGPR per row instead of a 64-bit pointer, no 64-bit
// VALU address arithmetic, and an access is masked by an out-of-range voffset instead of a branch.  AUX: the cache policy.
template <typename R> struct Buf;
template <> struct Buf<float> {
    template <int AUX = 0> static __device__ __forceinline__ float ld(rsrc_t r, unsigned vo, unsigned so) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, AUX)); }
    template <int AUX = 0> static __device__ __forceinline__ void st(rsrc_t r, unsigned vo, unsigned so, float v) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, vo, so, AUX); }
};
template <> struct Buf<double> {
    template <int AUX = 0> static __device__ __forceinline__ double ld(rsrc_t r, unsigned vo, unsigned so) { return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, AUX)); }
    template <int AUX = 0> static __device__ __forceinline__ void st(rsrc_t r, unsigned vo, unsigned so, double v) { __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, vo, so, AUX); }
};
#define BUF_OOB 0xFFFFFFFFu      // voffset >= num_records: the hardware drops the store / returns 0 for the load

// reciprocal: v_rcp_f32 (1 ulp) + one Newton step
__device__ __forceinline__ float recip_refined(float y)
{
    float r = __builtin_amdgcn_rcpf(y);
    const float e = __builtin_fmaf(-y, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}
